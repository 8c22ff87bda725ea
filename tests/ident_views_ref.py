"""Identifying enrolled subjects across the views of a rig (include/depthhead_hip.h, "identifying enrolled
subjects across the views of a rig") restated in numpy and plain Python: the six tests of taking part in their order, the score of
an (instance, subject) pair -- view_fit_ref.fit with a zero coarse count over the frames of the instance's set --, section 27's
decision (ident_ref.decide, reused as it is), the outputs, and the driver.  f64 with every operation rounded on its own; the sums
are view_fit_ref's Python ints.  Written from the header text, not from the kernels.  test_ident_views_ref.py holds it to scenes
whose answer is known; test_gpu_ident_views.py holds the GPU to it with no tolerance."""
import numpy as np

import fit_ref as fr
import ident_ref as ir
import view_fit_ref as vr
from fit_ref import F64
from ident_ref import AMBIGUOUS, FAR, NO_CANDIDATE, OK, RECORD_DTYPE, SKIPPED, UNKNOWN, mean_square  # noqa: F401

DEFAULT_MAX_RMS = 2.58              # DH_IDENT_VIEWS_DEFAULT_MAX_RMS
MAX_POINTS = 32768                  # DH_FIT_MAX_POINTS
# dh_view_fit_record, 32 bytes
SCORE_DTYPE = np.dtype([("points", "<u4"), ("steps", "<u4"), ("status", "<u4"), ("reserved", "<u4"), ("sum_r2_fixed", "<i8"), ("views_used", "<u8")])
assert SCORE_DTYPE.itemsize == 32


def params(iterations=4, min_points=64, gate=25.0, lam=1e-3, max_rms=DEFAULT_MAX_RMS, min_ratio=1.0):
    return ir.params(iterations, min_points, gate, lam, max_rms, min_ratio)


def why_not(inst, st_index, n, n_sets, fit_status, n_points, radius, big):
    """TAKING PART: None where the instance takes part, else the number (1 .. 6) of the first test it fails."""
    views = int(inst["views"])
    if views == 0:
        return 1
    if int(inst["first_cam"]) + views.bit_length() - 1 >= n:
        return 2
    if st_index >= n_sets:
        return 3
    if fit_status is not None and int(fit_status) != fr.OK:
        return 4
    if not ir.takes_part(dict(inst, frame=0), 1, None, radius, big):      # section 18's and 20's tests of R, t and scale
        return 5
    if bin(views).count("1") * n_points > MAX_POINTS:
        return 6
    return None


def score(frames, Ks, Vs, us, pts, nrm, inst, prm):
    """THE SCORE of one pair over the frames [n, h, w] of the instance's set: (R f32, t f32, the fit's record)."""
    fit_prm = fr.params(coarse_iterations=0, iterations=prm["iterations"], gate=(prm["gate"], prm["gate"]), lam=prm["lambda"],
                        min_points=prm["min_points"])
    return vr.fit(frames, Ks, Vs, us, inst["first_cam"], inst["views"], pts, nrm, inst["R"], inst["t"], inst["scale"], fit_prm)


def identify(frames, Ks, Vs, us, st, instances, sets=None, n_subjects=None, enrolled=None, fit_status=None, prm=None):
    """dh_fit_identify_subjects_views*: (subjects u32 [m], RECORD_DTYPE [m], poses -- instance dicts --, SCORE_DTYPE [m, n_subjects]).
    frames [n_sets, n, h, w]; instances: dicts with first_cam, views, R, t, scale."""
    prm = prm or params()
    n_subjects = len(st) if n_subjects is None else n_subjects
    n_sets, n = frames.shape[:2]
    big = ir.largest(st)
    m = len(instances)
    subjects, records = np.full(m, UNKNOWN, np.uint32), np.zeros(m, RECORD_DTYPE)
    table = np.zeros((m, n_subjects), SCORE_DTYPE)
    poses = []
    for i, inst in enumerate(instances):
        rec = records[i]
        rec["best"] = rec["second"] = UNKNOWN
        poses.append(dict(inst))
        si = 0 if sets is None else int(sets[i])
        if why_not(inst, si, n, n_sets, None if fit_status is None else fit_status[i], st.pts.shape[1], st.radius, big) is not None:
            rec["status"] = SKIPPED
            continue
        row, fitted = [None] * n_subjects, [None] * n_subjects
        for s in range(n_subjects):
            if enrolled is not None and not enrolled[s]:
                continue
            R, t, r = score(frames[si], Ks, Vs, us, st.pts[s], st.nrm[s], inst, prm)
            row[s], fitted[s] = r, (R, t)
            table[i, s] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"], r["views_used"])
        status, best, second, eligible = ir.decide(row, prm)
        rec["status"], rec["eligible"] = status, eligible
        if best is not None:
            rec["best"], rec["points_best"], rec["sum_r2_best"] = best, row[best]["points"], row[best]["sum_r2_fixed"]
            poses[i] = dict(inst, R=fitted[best][0], t=fitted[best][1])
        if second is not None:
            rec["second"], rec["points_second"], rec["sum_r2_second"] = second, row[second]["points"], row[second]["sum_r2_fixed"]
        if status == OK:
            subjects[i] = best
    return subjects, records, poses, table


def recognise_subjects_views(frames, Ks, Vs, us, st, starts, model, enrolled=None, fit_prm=None, ident_prm=None):
    """fit.recognise_subjects_views restated for one moment of the rig, frames [n, h, w]: every start fitted with `model` (points,
    normals) -- the generic head -- over its views, then identify from those instances and records with one set.  Returns
    (subjects, records, poses, the generic fit's records -- dicts)."""
    inst, recs = [], []
    for s in starts:
        R, t, rec = vr.fit(frames, Ks, Vs, us, s["first_cam"], s["views"], model[0], model[1], s["R"], s["t"], s["scale"], fit_prm)
        inst.append(dict(s, R=R, t=t))
        recs.append(rec)
    subjects, records, poses, _ = identify(frames[None], Ks, Vs, us, st, inst, None, None, enrolled, [r["status"] for r in recs], ident_prm)
    return subjects, records, poses, recs
