"""The shape step of DESIGN.md section 20 (include/depthhead_hip.h, "adapting a model's shape to a subject") restated in numpy:
f64 arithmetic with every product, sum and quotient rounded on its own, the fixed-point sums kept in Python ints, the fit's
elimination.  Written from the header text, not from the kernel.  The header defines a point's p, nrm, skip tests, pixel, d and
residual by reference to the fit's one pass, so those lines follow fit_ref.one_pass expression for expression (which hands out
sums, not points: test_shape_ref.py holds the two to the same e and count), and the sums' cast and the solve are fit_ref's own.
test_gpu_fit_shape.py holds the GPU to this byte for byte and test_shape_ref.py holds it to scenes whose answer is known."""
import numpy as np

import fit_ref as fr
from fit_ref import F64, S

OK, FEW_POINTS, SINGULAR = 0, 1, 2
SKIP = 0xFFFFFFFF
MAX_FIELDS = 8
# dh_shape_record, 88 bytes without padding
RECORD_DTYPE = np.dtype([("delta", "<f8", (8,)), ("points", "<u4"), ("instances", "<u4"), ("status", "<u4"), ("reserved", "<u4"),
                         ("sum_r2_fixed", "<i8")])
assert RECORD_DTYPE.itemsize == 88


def params(gate=25.0, lam=1e-3, min_points=64):
    return {"gate": float(gate), "lambda": float(lam), "min_points": int(min_points)}


def point_terms(frame, K, pts, nrm, scale, R, t, gate):
    """The fit's one pass at (R, t), per point: (passed [n] bool, nrm [3][n], residual [n])."""
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
    return ok, n, res


def instance_sums(frame, K, pts, nrm, basis, inst, gate):
    """(A {(k, l): int}, b [K] ints, e, count) of one instance (a record of dh_render_instance's fields, or a dict)."""
    R = np.asarray(inst["R"], dtype=np.float32).reshape(3, 3).astype(F64)
    t = np.asarray(inst["t"], dtype=np.float32).reshape(3).astype(F64)
    scale = F64(np.float32(inst["scale"]))
    ok, n, res = point_terms(frame, K, pts, nrm, scale, R, t, gate)
    B = np.asarray(basis, dtype=np.float32).astype(F64)
    J = []
    with np.errstate(all="ignore"):
        for k in range(len(B)):
            sb = B[k] * scale
            w = [(R[j, 0] * sb[:, 0] + R[j, 1] * sb[:, 1]) + R[j, 2] * sb[:, 2] for j in range(3)]
            J.append(((n[0] * w[0] + n[1] * w[1]) + n[2] * w[2])[ok])
    res = res[ok]
    A = {(k, l): fr._isum(J[k] * J[l]) for k in range(len(B)) for l in range(k, len(B))}
    b = [fr._isum(J[k] * res) for k in range(len(B))]
    return A, b, fr._isum(res * res), int(ok.sum())


def solve_subject(A, b, e, count, used, nk, prm):
    """One dh_shape_record from a subject's sums."""
    rec = np.zeros((), RECORD_DTYPE)
    rec["points"], rec["instances"], rec["sum_r2_fixed"] = count, used, e
    if count < prm["min_points"]:
        rec["status"] = FEW_POINTS
        return rec
    lam1 = F64(1.0) + F64(prm["lambda"])
    M = [[F64(0.0)] * nk for _ in range(nk)]
    for (k, l), v in A.items():
        M[k][l] = M[l][k] = F64(v) / S
    for k in range(nk):
        M[k][k] = M[k][k] * lam1 + 1e-9
    x = fr.solve(M, [F64(v) / S for v in b], nk)
    if x is None:
        rec["status"] = SINGULAR
        return rec
    rec["delta"][:nk] = x
    return rec


def shape_step(frames, Ks, pts, nrm, basis, instances, subjects=None, n_subjects=1, prm=None):
    """One shape step: RECORD_DTYPE [n_subjects].  Ks is one K [3, 3] or one per frame [n, 3, 3]."""
    prm = prm or params()
    Ks = np.asarray(Ks, dtype=np.float32)
    nk = len(basis)
    sums = [[{(k, l): 0 for k in range(nk) for l in range(k, nk)}, [0] * nk, 0, 0, 0] for _ in range(n_subjects)]
    for i, inst in enumerate(instances):
        sj = 0 if subjects is None else int(subjects[i])
        if sj == SKIP:
            continue
        f = int(inst["frame"])
        A, b, e, count = instance_sums(frames[f], Ks if Ks.ndim == 2 else Ks[f], pts, nrm, basis, inst, prm["gate"])
        s = sums[sj]
        for key, v in A.items():
            s[0][key] += v
        s[1] = [p + q for p, q in zip(s[1], b)]
        s[2] += e
        s[3] += count
        s[4] += 1 if count > 0 else 0
    out = np.zeros(n_subjects, RECORD_DTYPE)
    for sj, (A, b, e, count, used) in enumerate(sums):
        out[sj] = solve_subject(A, b, e, count, used, nk, prm)
    return out


def deform(verts, basis, coeffs):
    """v_i + sum_k c_k B_k[i] in f64, the fields added in index order, rounded to f32 once."""
    v = np.asarray(verts, dtype=np.float32).astype(F64)
    B = np.asarray(basis, dtype=np.float32).astype(F64)
    for k in range(len(B)):
        v = v + F64(coeffs[k]) * B[k]
    return v.astype(np.float32)


def adapt(frames, K, verts, tris, basis, starts, normals_of, rounds=6, fit_prm=None, shape_prm=None):
    """fit.adapt restated on fit_ref.fit: `starts` a list of instance dicts (frame, R, t, scale), `normals_of(verts, tris)` the
    caller's normals.  Returns (coefficients [K] f64, the last instances, trace of (coefficients, fit records, shape record))."""
    c = np.zeros(len(basis), F64)
    inst = [dict(s) for s in starts]
    trace = []
    for _ in range(rounds):
        v = deform(verts, basis, c)
        nrm = normals_of(v, tris)
        recs = []
        for s in inst:
            R, t, rec = fr.fit(frames[s["frame"]], K, v, nrm, s["R"], s["t"], s["scale"], fit_prm)
            s["R"], s["t"] = R, t
            recs.append(rec)
        subj = [0 if r["status"] == fr.OK else SKIP for r in recs]
        srec = shape_step(frames, K, v, nrm, basis, inst, subj, 1, shape_prm)[0]
        trace.append((c.copy(), recs, srec))
        if srec["status"] == OK:
            c = c + srec["delta"][:len(c)]
    return c, inst, trace
