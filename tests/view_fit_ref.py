"""The multi-view fitting rule of DESIGN.md section 21 (include/depthhead_hip.h, "fitting one model to several views") restated
in numpy, one instance at a time: per view the composite camera pose, section 18's per-point rule at it, the world row
J = (V^T nrm, V^T m), the 29 fixed-point sums over all (view, point) pairs in Python ints, and section 18's step and schedule
on the world pose (fit_ref.solve, fit_ref.cayley).  Written from the header text, not from the kernel; test_gpu_fit_views.py
holds the GPU to it byte for byte and test_view_fit_ref.py holds it to scenes whose answer is known."""
import numpy as np

from fit_ref import F64, FEW_POINTS, OK, PAIRS, S, SINGULAR, _isum, cayley, params, solve  # noqa: F401


def composite(V, u, R, t):
    """(R_v, t_v) of one view, in the header's element order."""
    Rv, tv = np.empty((3, 3), F64), np.empty(3, F64)
    for i in range(3):
        for j in range(3):
            Rv[i, j] = (V[i, 0] * R[0, j] + V[i, 1] * R[1, j]) + V[i, 2] * R[2, j]
        tv[i] = ((V[i, 0] * t[0] + V[i, 1] * t[1]) + V[i, 2] * t[2]) + u[i]
    return Rv, tv


def view_pass(frame, K, V, pts, nrm, scale, Rv, tv, gate):
    """(A[21], b[6], e, count) as Python ints, of one view of a pass: section 18's rule at (R_v, t_v), rows turned by V^T."""
    h, w = frame.shape
    K = np.asarray(K, dtype=np.float32).reshape(3, 3).astype(F64)
    v, m = np.asarray(pts, dtype=np.float32).astype(F64), np.asarray(nrm, dtype=np.float32).astype(F64)
    with np.errstate(all="ignore"):
        sv = v * F64(scale)
        p = [((Rv[j, 0] * sv[:, 0] + Rv[j, 1] * sv[:, 1]) + Rv[j, 2] * sv[:, 2]) + tv[j] for j in range(3)]
        n = [(Rv[j, 0] * m[:, 0] + Rv[j, 1] * m[:, 1]) + Rv[j, 2] * m[:, 2] for j in range(3)]
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
        q = [p[j] - tv[j] for j in range(3)]
        mm = [q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0]]
        J = [(V[0, j] * n[0] + V[1, j] * n[1]) + V[2, j] * n[2] for j in range(3)]
        J += [(V[0, j] * mm[0] + V[1, j] * mm[1]) + V[2, j] * mm[2] for j in range(3)]
    J = [j[ok] for j in J]
    res = res[ok]
    A = [_isum(J[a] * J[b]) for a, b in PAIRS]
    b = [_isum(J[a] * res) for a in range(6)]
    return A, b, _isum(res * res), int(ok.sum())


def one_pass(frames, Ks, Vs, us, first_cam, views, pts, nrm, scale, R, t, gate):
    """(A[21], b[6], e, count, views_used) of one pass at the world pose (R, t) over the set bits of `views`, ascending."""
    A, b, e, count, used = [0] * 21, [0] * 6, 0, 0, 0
    for k in range(64):
        if not (views >> k) & 1:
            continue
        c = first_cam + k
        V = np.asarray(Vs[c], dtype=np.float32).reshape(3, 3).astype(F64)
        u = np.asarray(us[c], dtype=np.float32).reshape(3).astype(F64)
        Rv, tv = composite(V, u, R, t)
        Ak, bk, ek, ck = view_pass(frames[c], Ks[c], V, pts, nrm, scale, Rv, tv, gate)
        A = [x + y for x, y in zip(A, Ak)]
        b = [x + y for x, y in zip(b, bk)]
        e, count = e + ek, count + ck
        if ck:
            used |= 1 << k
    return A, b, e, count, used


def fit(frames, Ks, Vs, us, first_cam, views, pts, nrm, R0, t0, scale=1.0, prm=None):
    """One instance.  frames [n, h, w], Ks [n, 3, 3], Vs [n, 3, 3], us [n, 3].  Returns (R [3, 3] f32, t [3] f32, record dict:
    points, steps, status, sum_r2_fixed, views_used)."""
    prm = prm or params()
    first_cam, views = int(first_cam), int(views)
    R = np.asarray(R0, dtype=np.float32).reshape(3, 3).astype(F64)
    t = np.asarray(t0, dtype=np.float32).reshape(3).astype(F64)
    scale = F64(np.float32(scale))
    lam1 = F64(1.0) + F64(prm["lambda"])
    steps, status = 0, OK
    schedule = [(3, prm["gate"][0])] * prm["coarse_iterations"] + [(6, prm["gate"][1])] * prm["iterations"]
    i = 0
    while i < len(schedule):
        n, gate = schedule[i]
        A, b, _, count, _ = one_pass(frames, Ks, Vs, us, first_cam, views, pts, nrm, scale, R, t, gate)
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
    _, _, e, count, used = one_pass(frames, Ks, Vs, us, first_cam, views, pts, nrm, scale, R, t, prm["gate"][1])
    return R.astype(np.float32), t.astype(np.float32), {"points": count, "steps": steps, "status": status, "sum_r2_fixed": e,
                                                         "views_used": used}
