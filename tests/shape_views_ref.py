"""The multi-view shape step of DESIGN.md section 23 (include/depthhead_hip.h, "adapting a model's shape across views") restated
in numpy.  Written from the header text, not from the kernel, out of the pieces the header names: the composite camera pose of a
view is view_fit_ref.composite, a view's per-point pass is shape_ref.point_terms at it, the products are section 20's with R_v
for R, the fixed-point sums are Python ints and the solve is shape_ref.solve_subject.  `used` counts (instance, view) pairs.
adapt_views restates fit.adapt_views on view_fit_ref.fit.  test_gpu_fit_shape_views.py holds the GPU to this byte for byte and
test_shape_views_ref.py holds it to scenes whose answer is known."""
import numpy as np

import fit_ref as fr
import shape_ref as sr
import view_fit_ref as vr
from fit_ref import F64
from shape_ref import FEW_POINTS, OK, RECORD_DTYPE, SINGULAR, SKIP, params  # noqa: F401


def pair_sums(frame, K, pts, nrm, basis, scale, Rv, tv, gate):
    """(A {(k, l): int}, b [K] ints, e, count) of one (instance, view) pair at the composite pose (R_v, t_v), f64."""
    ok, n, res = sr.point_terms(frame, K, pts, nrm, scale, Rv, tv, gate)
    B = np.asarray(basis, dtype=np.float32).astype(F64)
    J = []
    with np.errstate(all="ignore"):
        for k in range(len(B)):
            sb = B[k] * scale
            w = [(Rv[j, 0] * sb[:, 0] + Rv[j, 1] * sb[:, 1]) + Rv[j, 2] * sb[:, 2] for j in range(3)]
            J.append(((n[0] * w[0] + n[1] * w[1]) + n[2] * w[2])[ok])
    res = res[ok]
    A = {(k, l): fr._isum(J[k] * J[l]) for k in range(len(B)) for l in range(k, len(B))}
    b = [fr._isum(J[k] * res) for k in range(len(B))]
    return A, b, fr._isum(res * res), int(ok.sum())


def takes_part(inst, st, sj, n, n_sets, n_subjects):
    """The whole-instance test of the header for what a restatement can hold (the device's skips): a subject that is SKIP or
    beyond n_subjects, no view, a bit naming a camera >= n, a set >= n_sets, a non-finite pose."""
    views = int(inst["views"])
    if sj >= n_subjects or views == 0 or st >= n_sets:
        return False
    if int(inst["first_cam"]) + views.bit_length() - 1 >= n:
        return False
    return bool(np.isfinite(np.asarray(inst["R"], np.float64)).all() and np.isfinite(np.asarray(inst["t"], np.float64)).all()
                and np.isfinite(np.float64(inst["scale"])))


def shape_step(frames, Ks, Vs, us, pts, nrm, basis, instances, sets=None, subjects=None, n_subjects=1, prm=None):
    """One multi-view shape step: RECORD_DTYPE [n_subjects].  frames [n_sets, n, h, w], Ks [n, 3, 3], Vs [n, 3, 3], us [n, 3];
    instances: records or dicts with first_cam, views, R, t, scale."""
    prm = prm or params()
    n_sets, n = frames.shape[:2]
    nk = len(basis)
    sums = [[{(k, l): 0 for k in range(nk) for l in range(k, nk)}, [0] * nk, 0, 0, 0] for _ in range(n_subjects)]
    for i, inst in enumerate(instances):
        sj = 0 if subjects is None else int(subjects[i])
        st = 0 if sets is None else int(sets[i])
        if not takes_part(inst, st, sj, n, n_sets, n_subjects):
            continue
        R = np.asarray(inst["R"], dtype=np.float32).reshape(3, 3).astype(F64)
        t = np.asarray(inst["t"], dtype=np.float32).reshape(3).astype(F64)
        scale = F64(np.float32(inst["scale"]))
        first, views = int(inst["first_cam"]), int(inst["views"])
        s = sums[sj]
        for k in range(64):
            if not (views >> k) & 1:
                continue
            c = first + k
            V = np.asarray(Vs[c], dtype=np.float32).reshape(3, 3).astype(F64)
            u = np.asarray(us[c], dtype=np.float32).reshape(3).astype(F64)
            Rv, tv = vr.composite(V, u, R, t)
            A, b, e, count = pair_sums(frames[st, c], Ks[c], pts, nrm, basis, scale, Rv, tv, prm["gate"])
            for key, v in A.items():
                s[0][key] += v
            s[1] = [p + q for p, q in zip(s[1], b)]
            s[2] += e
            s[3] += count
            s[4] += 1 if count > 0 else 0
    out = np.zeros(n_subjects, RECORD_DTYPE)
    for sj, (A, b, e, count, used) in enumerate(sums):
        out[sj] = sr.solve_subject(A, b, e, count, used, nk, prm)
    return out


def adapt_views(frames, Ks, Vs, us, verts, tris, basis, starts, sets, normals_of, rounds=6, fit_prm=None, shape_prm=None):
    """fit.adapt_views restated on view_fit_ref.fit: `starts` a list of instance dicts (first_cam, views, R, t, scale), sets the
    set of each.  Returns (coefficients [K] f64, the last instances, trace of (coefficients, fit records, shape record))."""
    c = np.zeros(len(basis), F64)
    inst = [dict(s) for s in starts]
    sets = [0] * len(inst) if sets is None else [int(s) for s in sets]
    trace = []
    for _ in range(rounds):
        v = sr.deform(verts, basis, c)
        nrm = normals_of(v, tris)
        recs = []
        for s, st in zip(inst, sets):
            R, t, rec = vr.fit(frames[st], Ks, Vs, us, s["first_cam"], s["views"], v, nrm, s["R"], s["t"], s["scale"], fit_prm)
            s["R"], s["t"] = R, t
            recs.append(rec)
        subj = [0 if r["status"] == fr.OK else SKIP for r in recs]
        srec = shape_step(frames, Ks, Vs, us, v, nrm, basis, inst, sets, subj, 1, shape_prm)[0]
        trace.append((c.copy(), recs, srec))
        if srec["status"] == OK:
            c = c + srec["delta"][:len(c)]
    return c, inst, trace
