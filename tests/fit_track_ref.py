"""The rule of DESIGN.md section 19 (include/depthhead_hip.h, "carrying each camera's fitted pose across steps") restated in numpy,
one camera at a time, written from the header text: detection validity in Python ints, the start (the carried instance, its
constant-velocity variant in f32, or the forest's pose through the 120-entry angle table and two f64 matrix products), the fit
of tests/fit_ref.py with the start's own schedule, acceptance, and the state update.  It takes the poses, the support records
and the angle table as inputs -- it needs no forest and computes no cosine or sine of its own.  test_gpu_fit_tracker.py holds
the GPU to it byte for byte; test_fit_track_ref.py holds it to scenes whose answer is known."""
import numpy as np

import fit_ref as fr

F32, F64 = np.float32, np.float64
NONE, FITTED, CARRIED, REJECTED, ABSENT = 0, 1, 2, 3, 4
BAD_STATUS, BAD_POINTS, BAD_RMS, BAD_JUMP = 0x100, 0x200, 0x400, 0x800
MOTION = 1
U32_MAX = 0xFFFFFFFF

STATE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("t_prev", "<f4", (3,)), ("tracked", "<u4"), ("have_prev", "<u4"),
                  ("age", "<u4"), ("lost", "<u4")])
INSTANCE = np.dtype([("frame", "<u4"), ("mesh", "<u4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"), ("flags", "<u4")])
FIT = np.dtype([("points", "<u4"), ("steps", "<u4"), ("status", "<u4"), ("reserved", "<u4"), ("sum_r2_fixed", "<i8")])
RECORD = np.dtype([("instance", INSTANCE), ("fit", FIT), ("status", "<u4"), ("age", "<u4"), ("lost", "<u4"), ("reserved", "<u4")])
assert STATE.itemsize == 76 and RECORD.itemsize == 104


def params(iterations_tracked=6, keep_points=30, rms_max=5.0, max_jump=150.0, conf=(1, 50), min_windows=1, max_coast=3):
    return {"iterations_tracked": int(iterations_tracked), "keep_points": int(keep_points), "rms_max": float(rms_max),
            "max_jump": float(max_jump), "conf_num": int(conf[0]), "conf_den": int(conf[1]), "min_windows": int(min_windows),
            "max_coast": int(max_coast)}


def _sat(v):
    return min(int(v) + 1, U32_MAX)


def valid(sup, prm):
    mass, total = int(sup["mass"]), int(sup["total_mass"])
    return total > 0 and mass * prm["conf_den"] >= total * prm["conf_num"] and int(sup["windows"]) >= prm["min_windows"]


def angle_index(rotation):
    with np.errstate(all="ignore"):
        x = F64(rotation) / F64(3.14159) * F64(60.0) + F64(60.5)
    if not x >= 0.0:
        return 0
    return 119 if x >= 119.0 else int(x)


def _mul(A, B):
    o = np.empty((3, 3), F64)
    for i in range(3):
        for j in range(3):
            o[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
    return o


def forest_rotation(rotation, angles):
    """R [9] f32 of a pose's three angles through the table `angles` [120, 2] (cos, sin)."""
    tab = np.asarray(angles, F64).reshape(120, 2)
    (c0, s0), (c1, s1), (c2, s2) = (tab[angle_index(r)] for r in np.asarray(rotation, F64).reshape(3))
    z, one = F64(0.0), F64(1.0)
    Z = np.array([[c0, s0, z], [-s0, c0, z], [z, z, one]], F64)
    Y = np.array([[c1, z, s1], [z, one, z], [-s1, z, c1]], F64)
    X = np.array([[one, z, z], [z, c2, -s2], [z, s2, c2]], F64)
    return _mul(X, _mul(Y, Z)).astype(F32).reshape(9)


def step_camera(state, c, frame, K, pts, nrm, scale, flags, prm, fit_prm, present, pose, sup, angles):
    """One step of camera c.  `state`: a STATE scalar, changed in place.  Returns a RECORD scalar."""
    rec = np.zeros((), RECORD)
    st = state
    if not present:
        st["lost"] = _sat(st["lost"])
        st["have_prev"] = 0
        if int(st["lost"]) > prm["max_coast"]:
            st["tracked"], st["age"] = 0, 0
        rec["status"] = ABSENT
    else:
        ok = valid(sup, prm)
        if st["tracked"]:
            R = st["R"].copy()
            if (flags & MOTION) and st["have_prev"]:
                with np.errstate(all="ignore"):
                    t = (st["t"] + (st["t"] - st["t_prev"])).astype(F32)          # f32 throughout
            else:
                t = st["t"].copy()
            sched, carried = (0, prm["iterations_tracked"]), True
        elif ok:
            R, t = forest_rotation(pose["rotation"], angles), np.asarray(pose["mid_point"], F32).copy()
            sched, carried = (fit_prm["coarse_iterations"], fit_prm["iterations"]), False
        else:
            sched = None
        if sched is None:
            st["lost"] = _sat(st["lost"])
            st["tracked"], st["have_prev"], st["age"] = 0, 0, 0
            rec["status"] = NONE
        else:
            start = np.zeros((), INSTANCE)
            start["frame"], start["R"], start["t"], start["scale"] = c, R, t, F32(scale)
            p = dict(fit_prm, coarse_iterations=sched[0], iterations=sched[1])
            Rf, tf, r = fr.fit(frame, K, pts, nrm, R.reshape(3, 3), t, F32(scale), p)
            why = 0
            if r["status"] != fr.OK:
                why |= BAD_STATUS
            if r["points"] < prm["keep_points"]:
                why |= BAD_POINTS
            if r["sum_r2_fixed"] > int(F64(prm["rms_max"]) * F64(prm["rms_max"]) * F64(1048576.0)) * r["points"]:
                why |= BAD_RMS
            if ok:
                with np.errstate(all="ignore"):
                    d = tf.astype(F64) - np.asarray(pose["mid_point"], F32).astype(F64)
                    if not (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= F64(prm["max_jump"]) * F64(prm["max_jump"]):
                        why |= BAD_JUMP
            rec["fit"] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"])
            if why == 0:
                st["t_prev"] = st["t"]
                st["R"], st["t"] = Rf.reshape(9), tf
                st["have_prev"] = st["tracked"]
                st["tracked"], st["age"], st["lost"] = 1, _sat(st["age"]), 0
                rec["instance"] = start
                rec["instance"]["R"], rec["instance"]["t"] = Rf.reshape(9), tf
                rec["status"] = CARRIED if carried else FITTED
            else:
                st["tracked"], st["have_prev"], st["age"] = 0, 0, 0
                st["lost"] = _sat(st["lost"])
                rec["instance"] = start
                rec["status"] = REJECTED | why
    rec["age"], rec["lost"] = st["age"], st["lost"]
    return rec


class Tracker:
    """The state of n cameras and the step over all of them."""

    def __init__(self, Ks, pts, nrm, angles, scale=1.0, flags=0, prm=None):
        self.Ks = np.asarray(Ks, F32).reshape(-1, 3, 3)
        self.n = len(self.Ks)
        self.pts, self.nrm, self.angles = pts, nrm, np.asarray(angles, F64).reshape(120, 2)
        self.scale, self.flags, self.prm = scale, flags, prm or params()
        self.state = np.zeros(self.n, STATE)

    def reset(self, camera=None):
        if camera is None:
            self.state[:] = 0
        else:
            self.state[camera] = 0

    def step(self, frames, poses, support, present=None, fit_prm=None):
        fit_prm = fit_prm or fr.params()
        out = np.zeros(self.n, RECORD)
        for c in range(self.n):
            out[c] = step_camera(self.state[c], c, frames[c], self.Ks[c], self.pts, self.nrm, self.scale, self.flags, self.prm, fit_prm,
                                 present is None or bool(present[c]), poses[c], support[c], self.angles)
        return out
