"""Identifying the subject of a fitted head (include/depthhead_hip.h, "identifying the subject of a fitted
head") restated in numpy and plain Python: who takes part, the score of an (instance, subject) pair -- fit_ref.fit with a zero
coarse count --, the mean square, the order, the decision, the outputs, and the driver.  f64 with every operation rounded on its
own; the sums are fit_ref's Python ints.  Written from the header text, not from the kernels.  test_ident_ref.py holds it to
scenes whose answer is known; test_gpu_ident.py holds the GPU to it with no tolerance."""
import numpy as np

import fit_ref as fr
from fit_ref import F64, S

OK, SKIPPED, NO_CANDIDATE, FAR, AMBIGUOUS = 0, 1, 2, 3, 4
UNKNOWN = 0xFFFFFFFF
MAX_PAIRS = 1 << 22
DEFAULT_MAX_RMS = 1.68
R_TOLERANCE, MAX_EXTENT, MAX_FIELD = 0.02, 4096.0, 256.0       # DH_FIT_R_TOLERANCE, DH_FIT_MAX_EXTENT, DH_SHAPE_MAX_FIELD
# dh_ident_record, 40 bytes without padding; dh_fit_record, 24 bytes
RECORD_DTYPE = np.dtype([("status", "<u4"), ("best", "<u4"), ("second", "<u4"), ("eligible", "<u4"), ("points_best", "<u4"),
                         ("points_second", "<u4"), ("sum_r2_best", "<i8"), ("sum_r2_second", "<i8")])
SCORE_DTYPE = np.dtype([("points", "<u4"), ("steps", "<u4"), ("status", "<u4"), ("reserved", "<u4"), ("sum_r2_fixed", "<i8")])
assert RECORD_DTYPE.itemsize == 40 and SCORE_DTYPE.itemsize == 24


def params(iterations=4, min_points=64, gate=25.0, lam=1e-3, max_rms=DEFAULT_MAX_RMS, min_ratio=1.0):
    return {"iterations": int(iterations), "min_points": int(min_points), "gate": float(gate), "lambda": float(lam),
            "max_rms": float(max_rms), "min_ratio": float(min_ratio)}


def largest(st):
    """The basis's largest |B_k[i]| as the library computes it."""
    b = np.asarray(st.basis, np.float32).astype(F64).reshape(-1, 3)
    return np.sqrt(((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]).max())


def takes_part(inst, n_frames, fit_status, radius, big):
    """TAKING PART: the frame; the fit record; R, t and scale finite, |R R^T - I| <= 0.02 per element, |scale| * radius <= 4096,
    |scale| * largest <= 256.  A NaN fails each test."""
    if int(inst["frame"]) >= n_frames or (fit_status is not None and int(fit_status) != fr.OK):
        return False
    R = np.asarray(inst["R"], dtype=np.float32).reshape(3, 3).astype(F64)
    t = np.asarray(inst["t"], dtype=np.float32).reshape(3).astype(F64)
    scale = F64(np.float32(inst["scale"]))
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(scale)):
        return False
    for a in range(3):
        for b in range(a, 3):
            g = (R[a, 0] * R[b, 0] + R[a, 1] * R[b, 1]) + R[a, 2] * R[b, 2]
            if not abs(g - (1.0 if a == b else 0.0)) <= R_TOLERANCE:
                return False
    mag = abs(scale)
    return bool(mag * F64(radius) <= MAX_EXTENT and mag * F64(big) <= MAX_FIELD)


def score(frame, K, pts, nrm, inst, prm):
    """THE SCORE of one pair: (R f32, t f32, the fit's record)."""
    fit_prm = fr.params(coarse_iterations=0, iterations=prm["iterations"], gate=(prm["gate"], prm["gate"]), lam=prm["lambda"],
                        min_points=prm["min_points"])
    return fr.fit(frame, K, pts, nrm, inst["R"], inst["t"], inst["scale"], fit_prm)


def mean_square(sum_r2_fixed, points):
    return (F64(int(sum_r2_fixed)) / S) / F64(int(points))


def precedes(m_a, a, m_b, b):
    return bool(m_a < m_b or (m_a == m_b and a < b))


def decide(scores, prm):
    """THE DECISION of an instance that takes part, from its row of scores (dicts; None: the pair did not run):
    (status, best, second, eligible)."""
    E = [(mean_square(r["sum_r2_fixed"], r["points"]), s) for s, r in enumerate(scores)
         if r is not None and r["status"] == fr.OK and r["points"] >= prm["min_points"]]
    best = second = None
    for c in E:
        if best is None or precedes(*c, *best):
            best = c
    for c in E:
        if c is not best and (second is None or precedes(*c, *second)):
            second = c
    if best is None:
        return NO_CANDIDATE, None, None, 0
    max_ms = F64(prm["max_rms"]) * F64(prm["max_rms"])
    if not best[0] <= max_ms:
        status = FAR
    elif second is not None and not second[0] >= F64(prm["min_ratio"]) * best[0]:
        status = AMBIGUOUS
    else:
        status = OK
    return status, best[1], None if second is None else second[1], len(E)


def identify(frames, Ks, st, instances, n_subjects=None, enrolled=None, fit_status=None, prm=None):
    """dh_fit_identify_subjects*: (subjects u32 [m], RECORD_DTYPE [m], poses -- instance dicts --, SCORE_DTYPE [m, n_subjects])."""
    prm = prm or params()
    n_subjects = len(st) if n_subjects is None else n_subjects
    Ks = np.asarray(Ks, dtype=np.float32)
    big = largest(st)
    m = len(instances)
    subjects, records = np.full(m, UNKNOWN, np.uint32), np.zeros(m, RECORD_DTYPE)
    table = np.zeros((m, n_subjects), SCORE_DTYPE)
    poses = []
    for i, inst in enumerate(instances):
        rec = records[i]
        rec["best"] = rec["second"] = UNKNOWN
        poses.append(dict(inst))
        if not takes_part(inst, len(frames), None if fit_status is None else fit_status[i], st.radius, big):
            rec["status"] = SKIPPED
            continue
        f = int(inst["frame"])
        row, fitted = [None] * n_subjects, [None] * n_subjects
        for s in range(n_subjects):
            if enrolled is not None and not enrolled[s]:
                continue
            R, t, r = score(frames[f], Ks if Ks.ndim == 2 else Ks[f], st.pts[s], st.nrm[s], inst, prm)
            row[s], fitted[s] = r, (R, t)
            table[i, s] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"])
        status, best, second, eligible = decide(row, prm)
        rec["status"], rec["eligible"] = status, eligible
        if best is not None:
            rec["best"], rec["points_best"], rec["sum_r2_best"] = best, row[best]["points"], row[best]["sum_r2_fixed"]
            poses[i] = dict(inst, R=fitted[best][0], t=fitted[best][1])
        if second is not None:
            rec["second"], rec["points_second"], rec["sum_r2_second"] = second, row[second]["points"], row[second]["sum_r2_fixed"]
        if status == OK:
            subjects[i] = best
    return subjects, records, poses, table


def recognise_subjects(frames, K, st, starts, model, enrolled=None, fit_prm=None, ident_prm=None):
    """fit.recognise_subjects restated: every start fitted with `model` (points, normals) -- the generic head --, then identify
    from those poses and records.  Returns (subjects, records, poses, the generic fit's records -- dicts)."""
    inst, recs = [], []
    for s in starts:
        R, t, rec = fr.fit(frames[s["frame"]], K, model[0], model[1], s["R"], s["t"], s["scale"], fit_prm)
        inst.append(dict(s, R=R, t=t))
        recs.append(rec)
    subjects, records, poses, _ = identify(frames, K, st, inst, None, enrolled, [r["status"] for r in recs], ident_prm)
    return subjects, records, poses, recs
