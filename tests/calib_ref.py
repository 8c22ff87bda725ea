"""The calibration step of DESIGN.md section 24 (include/depthhead_hip.h, "calibrating a view table") restated in numpy.  Written
from the header text, not from the kernel, out of the pieces the header names: the composite camera pose of a view is
view_fit_ref.composite, the per-point pass follows fit_ref.one_pass expression for expression (which hands out sums, not points:
test_calib_ref.py holds the two to the same sums), the row is the fit's about the camera's pivot with the rotation columns in
units of ARM_UNIT, the fixed-point sums are Python ints, the solve and the Cayley rotation are fit_ref's.  calibrate_views
restates fit.calibrate_views on view_fit_ref.fit.  test_gpu_calibrate.py holds the GPU to this byte for byte and
test_calib_ref.py holds it to scenes whose answer is known."""
import numpy as np

import fit_ref as fr
import view_fit_ref as vr
from fit_ref import F64, PAIRS, S

OK, FEW_POINTS, SINGULAR, NOT_ORTHONORMAL, HELD = 0, 1, 2, 3, 4
SKIP = 0xFFFFFFFF
ARM_UNIT = 64.0
MAX_ARM = 2048.0
MAX_EXTENT = 4096.0
R_TOLERANCE = 0.02
VIEW_TOLERANCE = 0.001
# dh_calib_record, 120 bytes without padding
RECORD_DTYPE = np.dtype([("V", "<f4", (9,)), ("u", "<f4", (3,)), ("points", "<u4"), ("pairs", "<u4"), ("status", "<u4"), ("reserved", "<u4"),
                         ("sum_r2_fixed", "<i8"), ("delta", "<f8", (6,))])
assert RECORD_DTYPE.itemsize == 120


def params(gate=25.0, lam=1e-3, min_points=64, pivot=(0.0, 0.0, 0.0)):
    return {"gate": float(gate), "lambda": float(lam), "min_points": int(min_points), "pivot": tuple(float(v) for v in pivot)}


def pivot_of(V, u, o):
    """g_c: the camera-space image of the world point o, in the element order of t_v."""
    return np.array([((V[i, 0] * F64(o[0]) + V[i, 1] * F64(o[1])) + V[i, 2] * F64(o[2])) + u[i] for i in range(3)], F64)


def _gram_within(M, tol):
    """Whether every element of M M^T (f64, formed as section 18 forms R R^T) is within tol of the identity's; NaN fails."""
    for a in range(3):
        for b in range(a, 3):
            g = (M[a, 0] * M[b, 0] + M[a, 1] * M[b, 1]) + M[a, 2] * M[b, 2]
            if not abs(g - (1.0 if a == b else 0.0)) <= tol:
                return False
    return True


def takes_part(inst, st, tk, n, n_sets, radius):
    """The whole-instance test of the header (the device's skips): DH_CALIB_SKIP, no view, a bit naming a camera >= n, a set >=
    n_sets, a non-finite R, t or scale, an R outside DH_FIT_R_TOLERANCE, |scale| * radius above DH_FIT_MAX_EXTENT."""
    views = int(inst["views"])
    if tk == SKIP or views == 0 or int(inst["first_cam"]) + views.bit_length() - 1 >= n or st >= n_sets:
        return False
    R = np.asarray(inst["R"], np.float32).reshape(3, 3).astype(F64)
    t = np.asarray(inst["t"], np.float32).astype(F64)
    sc = F64(np.float32(inst["scale"]))
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(sc)):
        return False
    return _gram_within(R, R_TOLERANCE) and bool(abs(sc) * F64(radius) <= MAX_EXTENT)


def within_arm(tv, g):
    """The pair test: every |t_v[i] - g_c[i]| <= DH_CALIB_MAX_ARM (a NaN fails)."""
    with np.errstate(all="ignore"):
        return all(bool(abs(tv[i] - g[i]) <= MAX_ARM) for i in range(3))


def pair_sums(frame, K, pts, nrm, scale, Rv, tv, g, gate):
    """(A[21], b[6], e, count) as Python ints, of one (instance, view) pair at the composite pose (R_v, t_v) with pivot g."""
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
        q = [p[j] - g[j] for j in range(3)]
        J = [n[0], n[1], n[2], (q[1] * n[2] - q[2] * n[1]) / ARM_UNIT, (q[2] * n[0] - q[0] * n[2]) / ARM_UNIT,
             (q[0] * n[1] - q[1] * n[0]) / ARM_UNIT]
    J = [j[ok] for j in J]
    res = res[ok]
    A = [fr._isum(J[a] * J[b]) for a, b in PAIRS]
    b = [fr._isum(J[a] * res) for a in range(6)]
    return A, b, fr._isum(res * res), int(ok.sum())


def camera_sums(frames, Ks, Vs, us, pts, nrm, instances, sets=None, take=None, hold=None, prm=None):
    """The sums of every camera: a list of [A[21], b[6], e, count, pairs] of Python ints."""
    prm = prm or params()
    n_sets, n = frames.shape[:2]
    radius = float(np.sqrt((np.asarray(pts, np.float32).astype(F64) ** 2).sum(axis=1).max()))
    sums = [[[0] * 21, [0] * 6, 0, 0, 0] for _ in range(n)]
    for i, inst in enumerate(instances):
        st = 0 if sets is None else int(sets[i])
        tk = 0 if take is None else int(take[i])
        if not takes_part(inst, st, tk, n, n_sets, radius):
            continue
        R = np.asarray(inst["R"], dtype=np.float32).reshape(3, 3).astype(F64)
        t = np.asarray(inst["t"], dtype=np.float32).reshape(3).astype(F64)
        scale = F64(np.float32(inst["scale"]))
        first, views = int(inst["first_cam"]), int(inst["views"])
        for k in range(64):
            if not (views >> k) & 1:
                continue
            c = first + k
            if hold is not None and hold[c]:
                continue
            V = np.asarray(Vs[c], dtype=np.float32).reshape(3, 3).astype(F64)
            u = np.asarray(us[c], dtype=np.float32).reshape(3).astype(F64)
            Rv, tv = vr.composite(V, u, R, t)
            g = pivot_of(V, u, prm["pivot"])
            if not within_arm(tv, g):
                continue
            A, b, e, count = pair_sums(frames[st, c], Ks[c], pts, nrm, scale, Rv, tv, g, prm["gate"])
            s = sums[c]
            s[0] = [x + y for x, y in zip(s[0], A)]
            s[1] = [x + y for x, y in zip(s[1], b)]
            s[2] += e
            s[3] += count
            s[4] += 1 if count > 0 else 0
    return sums


def solve_camera(V32, u32, A, b, e, count, pairs, held, prm):
    """One dh_calib_record from a camera's sums and its entry (V32 [3, 3] f32, u32 [3] f32)."""
    rec = np.zeros((), RECORD_DTYPE)
    rec["V"], rec["u"] = np.asarray(V32, np.float32).reshape(9), np.asarray(u32, np.float32).reshape(3)
    rec["points"], rec["pairs"], rec["sum_r2_fixed"] = count, pairs, e
    if held:
        rec["status"] = HELD
        return rec
    if count < prm["min_points"]:
        rec["status"] = FEW_POINTS
        return rec
    lam1 = F64(1.0) + F64(prm["lambda"])
    M = [[F64(0.0)] * 6 for _ in range(6)]
    for (a, c), v in zip(PAIRS, A):
        M[a][c] = M[c][a] = F64(v) / S
    for a in range(6):
        M[a][a] = M[a][a] * lam1 + 1e-9
    x = fr.solve(M, [F64(v) / S for v in b], 6)
    if x is None:
        rec["status"] = SINGULAR
        return rec
    V = np.asarray(V32, np.float32).reshape(3, 3).astype(F64)
    u = np.asarray(u32, np.float32).reshape(3).astype(F64)
    g = pivot_of(V, u, prm["pivot"])
    with np.errstate(all="ignore"):
        w = [x[3] / ARM_UNIT, x[4] / ARM_UNIT, x[5] / ARM_UNIT]
        V2 = fr.cayley(V, w)
        col = np.zeros((3, 3), F64)
        col[:, 0] = u - g                      # C s is the first column of C [s 0 0]: the header's (C0 s0 + C1 s1) + C2 s2
        Cs = fr.cayley(col, w)[:, 0]
        u2 = np.array([(Cs[i] + g[i]) + x[i] for i in range(3)], F64)
        Vf, uf = V2.astype(np.float32), u2.astype(np.float32)
    if not _gram_within(Vf.astype(F64), VIEW_TOLERANCE):
        rec["status"] = NOT_ORTHONORMAL
        return rec
    rec["V"], rec["u"] = Vf.reshape(9), uf
    rec["delta"][:3] = x[:3]
    rec["delta"][3:] = w
    return rec


def calib_step(frames, Ks, Vs, us, pts, nrm, instances, sets=None, take=None, hold=None, prm=None):
    """One calibration step: RECORD_DTYPE [n].  frames [n_sets, n, h, w], Ks [n, 3, 3], Vs [n, 3, 3], us [n, 3]; instances:
    records or dicts with first_cam, views, R, t, scale."""
    prm = prm or params()
    n = frames.shape[1]
    sums = camera_sums(frames, Ks, Vs, us, pts, nrm, instances, sets, take, hold, prm)
    out = np.zeros(n, RECORD_DTYPE)
    for c, (A, b, e, count, pairs) in enumerate(sums):
        out[c] = solve_camera(Vs[c], us[c], A, b, e, count, pairs, hold is not None and bool(hold[c]), prm)
    return out


def next_table(Vs, us, rec):
    """fit.views_from_records' arrays: the OK records' entries, the old ones elsewhere."""
    V, u = np.array(Vs, np.float32).reshape(-1, 3, 3), np.array(us, np.float32).reshape(-1, 3)
    ok = rec["status"] == OK
    V[ok] = rec["V"][ok].reshape(-1, 3, 3)
    u[ok] = rec["u"][ok]
    return V, u


def calibrate_views(frames, Ks, V, u, pts, nrm, starts, sets=None, hold=None, steps=8, wide_steps=3, gates=(60.0, 25.0), rounds=3,
                    joint_steps=2, fit_prm=None, refit_prm=None, lam=1e-3, min_points=64):
    """fit.calibrate_views restated on view_fit_ref.fit: `starts` a list of instance dicts (first_cam, views, R, t, scale).
    Returns (V, u, the last instances, trace of {"stage", "records", "fit"})."""
    V, u = np.array(V, np.float32).reshape(-1, 3, 3), np.array(u, np.float32).reshape(-1, 3)
    n = len(V)
    inst = [dict(s) for s in starts]
    sets = [0] * len(inst) if sets is None else [int(s) for s in sets]
    hd = np.zeros(n, np.uint8) if hold is None else (np.asarray(hold).reshape(n) != 0).astype(np.uint8)
    refit_prm = refit_prm or fr.params(coarse_iterations=0, iterations=6)
    held_masks = []
    for s in inst:
        m = 0
        for k in range(64):
            c = int(s["first_cam"]) + k
            if (int(s["views"]) >> k) & 1 and c < n and hd[c]:
                m |= 1 << k
        held_masks.append(m)
    trace = []

    def fit_all(masks, prm):
        recs = []
        for s, st, m in zip(inst, sets, masks):
            if m == 0:
                recs.append({"points": 0, "steps": 0, "status": fr.FEW_POINTS, "sum_r2_fixed": 0, "views_used": 0})
                continue
            R, t, rec = vr.fit(frames[st], Ks, V, u, s["first_cam"], m, pts, nrm, s["R"], s["t"], s["scale"], prm)
            s["R"], s["t"] = R, t
            recs.append(rec)
        return recs

    def calib(recs, gate, stage):
        nonlocal V, u
        ok = np.array([r["status"] == fr.OK for r in recs])
        ts = np.array([np.asarray(s["t"], np.float32) for s in inst], np.float32).reshape(-1, 3)
        pivot = ts[ok].astype(np.float64).mean(axis=0) if ok.any() else np.zeros(3)
        take = [0 if o else SKIP for o in ok]
        crec = calib_step(frames, Ks, V, u, pts, nrm, inst, sets, take, hd, params(gate, lam, min_points, pivot))
        trace.append({"stage": stage, "records": crec, "fit": recs})
        V, u = next_table(V, u, crec)

    recs = fit_all(held_masks, fit_prm)
    for k in range(steps):
        calib(recs, gates[0] if k < wide_steps else gates[1], "held")
    for r in range(rounds):
        recs = fit_all([int(s["views"]) for s in inst], refit_prm)
        for _ in range(joint_steps):
            calib(recs, gates[1], f"joint {r}")
    return V, u, inst, trace
