"""The fitting rule of DESIGN.md section 18 (include/depthhead_hip.h, "fitting posed models to depth frames") restated in numpy,
one instance at a time: f64 arithmetic with every product, sum and quotient rounded on its own, the 29 fixed-point sums kept
in Python ints, Gaussian elimination without pivoting, the Cayley update.  Written from the header text, not from the kernel;
test_gpu_fit.py holds the GPU to it byte for byte and test_fit_ref.py holds it to scenes whose answer is known."""
import numpy as np

F64 = np.float64
S = 1048576.0                      # 2^20
OK, FEW_POINTS, SINGULAR = 0, 1, 2
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]      # the 21 sums A_ab, a <= b, in this order


def params(coarse_iterations=6, iterations=14, gate=(120.0, 25.0), lam=1e-3, min_points=16):
    return {"coarse_iterations": int(coarse_iterations), "iterations": int(iterations), "gate": (float(gate[0]), float(gate[1])),
            "lambda": float(lam), "min_points": int(min_points)}


def _isum(x):
    """Sum of (int64)(x * 2^20), truncating, in Python ints."""
    return sum(int(v) for v in (x * S).tolist())


def one_pass(frame, K, pts, nrm, scale, R, t, gate):
    """(A[21], b[6], e, count) as Python ints, of one pass at pose (R, t) with gate `gate`."""
    h, w = frame.shape
    K = np.asarray(K, dtype=np.float32).reshape(3, 3).astype(F64)
    v, m = np.asarray(pts, dtype=np.float32).astype(F64), np.asarray(nrm, dtype=np.float32).astype(F64)
    with np.errstate(all="ignore"):
        sv = v * F64(scale)
        p = [((R[j, 0] * sv[:, 0] + R[j, 1] * sv[:, 1]) + R[j, 2] * sv[:, 2]) + t[j] for j in range(3)]
        n = [(R[j, 0] * m[:, 0] + R[j, 1] * m[:, 1]) + R[j, 2] * m[:, 2] for j in range(3)]
        ok = p[2] >= 1.0
        c = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]
        ok &= c < 0.0
        r = [(p[0] * K[j, 0] + p[1] * K[j, 1]) + p[2] * K[j, 2] for j in range(3)]
        x, y = r[0] / r[2], r[1] / r[2]
        ok &= (x >= 0.0) & (x < F64(w)) & (y >= 0.0) & (y < F64(h))
        px, py = np.where(ok, x, 0.0).astype(np.int64), np.where(ok, y, 0.0).astype(np.int64)
        d = frame[py, px].astype(F64)
        ok &= d != 0.0
        ok &= np.abs(d - p[2]) <= F64(gate)
        res = c * (d / p[2] - 1.0)
        q = [p[j] - t[j] for j in range(3)]
        J = [n[0], n[1], n[2], q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0]]
    J = [j[ok] for j in J]
    res = res[ok]
    A = [_isum(J[a] * J[b]) for a, b in PAIRS]
    b = [_isum(J[a] * res) for a in range(6)]
    return A, b, _isum(res * res), int(ok.sum())


def solve(A, b, n):
    """Gaussian elimination without pivoting in index order on the leading n x n block; None when a pivot is not > 0.0."""
    A = [[F64(A[i][j]) for j in range(n)] for i in range(n)]
    b = [F64(b[i]) for i in range(n)]
    with np.errstate(all="ignore"):
        for k in range(n):
            piv = A[k][k]
            if not piv > 0.0:
                return None
            for i in range(k + 1, n):
                f = A[i][k] / piv
                for j in range(k + 1, n):
                    A[i][j] = A[i][j] - f * A[k][j]
                b[i] = b[i] - f * b[k]
        x = [F64(0.0)] * n
        for i in range(n - 1, -1, -1):
            s = b[i]
            for j in range(i + 1, n):
                s = s - A[i][j] * x[j]
            x[i] = s / A[i][i]
    return x


def cayley(R, w):
    """R' = C R, C the Cayley rotation of a = w / 2, in the element order the header states."""
    a = [w[0] / 2.0, w[1] / 2.0, w[2] / 2.0]
    q = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    s, d = 1.0 + q, 1.0 - q
    a2 = [2.0 * a[0], 2.0 * a[1], 2.0 * a[2]]
    C = [[(d + a2[0] * a[0]) / s, (a2[0] * a[1] - a2[2]) / s, (a2[0] * a[2] + a2[1]) / s],
         [(a2[1] * a[0] + a2[2]) / s, (d + a2[1] * a[1]) / s, (a2[1] * a[2] - a2[0]) / s],
         [(a2[2] * a[0] - a2[1]) / s, (a2[2] * a[1] + a2[0]) / s, (d + a2[2] * a[2]) / s]]
    out = np.empty((3, 3), F64)
    for i in range(3):
        for j in range(3):
            out[i, j] = (C[i][0] * R[0, j] + C[i][1] * R[1, j]) + C[i][2] * R[2, j]
    return out


def fit(frame, K, pts, nrm, R0, t0, scale=1.0, prm=None):
    """One instance.  Returns (R [3, 3] f32, t [3] f32, record dict: points, steps, status, sum_r2_fixed)."""
    prm = prm or params()
    R = np.asarray(R0, dtype=np.float32).reshape(3, 3).astype(F64)
    t = np.asarray(t0, dtype=np.float32).reshape(3).astype(F64)
    scale = F64(np.float32(scale))
    lam1 = F64(1.0) + F64(prm["lambda"])
    steps, status = 0, OK
    schedule = [(3, prm["gate"][0])] * prm["coarse_iterations"] + [(6, prm["gate"][1])] * prm["iterations"]
    i = 0
    while i < len(schedule):
        n, gate = schedule[i]
        A, b, _, count = one_pass(frame, K, pts, nrm, scale, R, t, gate)
        if count < prm["min_points"]:
            status = FEW_POINTS
            break
        M = [[F64(0.0)] * 6 for _ in range(6)]
        for (a, c), v in zip(PAIRS, A):
            M[a][c] = M[c][a] = F64(v) / S
        for a in range(6):
            M[a][a] = M[a][a] * lam1 + 1e-9
        x = solve(M, [F64(v) / S for v in b], n)
        if x is None:
            status = SINGULAR
            break
        for j in range(3):
            t[j] = t[j] + x[j]
        if n == 6:
            R = cayley(R, x[3:6])
        steps += 1
        i += 1
        if all(abs(v) < 1e-6 for v in x):
            if n == 6:
                break
            i = prm["coarse_iterations"]          # a converged coarse step ends the coarse phase
    _, _, e, count = one_pass(frame, K, pts, nrm, scale, R, t, prm["gate"][1])
    return R.astype(np.float32), t.astype(np.float32), {"points": count, "steps": steps, "status": status, "sum_r2_fixed": e}
