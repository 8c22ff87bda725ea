"""The rule of DESIGN.md section 22 (include/depthhead_hip.h, "carrying each rig person's fitted world pose across steps")
restated in numpy, one rig at a time, written from the header text: the bind of persons to entries in Python ints and lists,
the start (the carried world pose, its constant-velocity variant in f32, or the person record's world with V_b^T times the
head's rotation through section 19's angle table: fit_track_ref.forest_rotation), the multi-view fit of tests/view_fit_ref.py
with the start's own schedule, acceptance, and the state update with counters as Python ints.  It takes heads, persons and
the angle table as inputs -- it needs no forest and computes no cosine or sine of its own.  test_gpu_rig_fit_tracker.py holds
the GPU to it byte for byte; test_rig_fit_track_ref.py holds it to scenes whose answer is known."""
import numpy as np

import fit_ref as fr
import fit_track_ref as ft
import view_fit_ref as vr
from fit_track_ref import ABSENT, BAD_JUMP, BAD_POINTS, BAD_RMS, BAD_STATUS, CARRIED, FITTED, MOTION, NONE, REJECTED  # noqa: F401

F32, F64 = np.float32, np.float64
U32_MAX = 0xFFFFFFFF
NO_PERSON = 0xFFFFFFFF
SLOTS = PERSONS = 16

STATE = np.dtype([("id", "<u4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("t_prev", "<f4", (3,)), ("views_used", "<u8"),
                  ("tracked", "<u4"), ("have_prev", "<u4"), ("age", "<u4"), ("lost", "<u4")])
INSTANCE = np.dtype([("first_cam", "<u4"), ("model", "<u4"), ("views", "<u8"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"),
                     ("flags", "<u4")])
FIT = np.dtype([("points", "<u4"), ("steps", "<u4"), ("status", "<u4"), ("reserved", "<u4"), ("sum_r2_fixed", "<i8"), ("views_used", "<u8")])
RECORD = np.dtype([("instance", INSTANCE), ("fit", FIT), ("id", "<u4"), ("status", "<u4"), ("age", "<u4"), ("lost", "<u4"),
                   ("person", "<u4"), ("reserved", "<u4")])
assert STATE.itemsize == 88 and INSTANCE.itemsize == 72 and FIT.itemsize == 32 and RECORD.itemsize == 128


def params(iterations_tracked=6, keep_points=30, rms_max=5.0, max_jump=150.0, max_coast=3, max_misses=3):
    return {"iterations_tracked": int(iterations_tracked), "keep_points": int(keep_points), "rms_max": float(rms_max),
            "max_jump": float(max_jump), "max_coast": int(max_coast), "max_misses": int(max_misses)}


def _sat(v):
    return min(int(v) + 1, U32_MAX)


def names_head(p, n_heads, max_heads):
    b = int(p["best_cam"])
    return b < len(n_heads) and int(p["best_head"]) < min(int(n_heads[b]), max_heads)


def bind(ids, tracked, persons, n_persons, n_heads, max_heads):
    """Step 1.  ids, tracked: the entries' (lists of 16 ints).  Returns (slots, new_ids, freed): slots[s] = ("seen", i) /
    ("unseen", None) / ("unbound", i) / None; new_ids the entries' ids after the bind (an entry a person founded has its id;
    such an entry starts from zeros); freed the unseen entries that were not tracked and are zeroed."""
    ids = [int(v) for v in ids]
    founded, holder, unbound = set(), {}, []
    for i in range(min(int(n_persons), PERSONS)):
        p = persons[i]
        if not names_head(p, n_heads, max_heads):
            continue
        pid = int(p["id"])
        if pid == 0:
            unbound.append(i)
        elif pid in ids:
            s = ids.index(pid)
            if s in holder:
                unbound.append(i)
            else:
                holder[s] = i
        elif 0 in ids:
            s = ids.index(0)
            ids[s] = pid
            founded.add(s)
            holder[s] = i
        else:
            unbound.append(i)
    slots, freed = [None] * SLOTS, set()
    for s in range(SLOTS):
        if s in holder:
            slots[s] = ("seen", holder[s])
        elif ids[s] != 0:
            if tracked[s] and s not in founded:
                slots[s] = ("unseen", None)
            else:
                freed.add(s)
                ids[s] = 0
    for i in unbound:
        free = [s for s in range(SLOTS) if slots[s] is None]
        if not free:
            break
        slots[free[0]] = ("unbound", i)
    return slots, ids, founded, freed


def detected_rotation(V, rotation, angles):
    """R [9] f32 = V^T Rh with Rh section 19's f32 rotation of the head's angles, widened."""
    Rh = ft.forest_rotation(rotation, angles).reshape(3, 3).astype(F64)
    V = np.asarray(V, F32).reshape(3, 3).astype(F64)
    R = np.empty((3, 3), F64)
    for i in range(3):
        for j in range(3):
            R[i, j] = (V[0, i] * Rh[0, j] + V[1, i] * Rh[1, j]) + V[2, i] * Rh[2, j]
    return R.astype(F32).reshape(9)


class Tracker:
    """The state of every rig and the step over all of them."""

    def __init__(self, Ks, Vs, us, rig_begin, pts, nrm, angles, scale=1.0, flags=0, prm=None):
        self.Ks = np.asarray(Ks, F32).reshape(-1, 3, 3)
        self.Vs, self.us = np.asarray(Vs, F32).reshape(-1, 3, 3), np.asarray(us, F32).reshape(-1, 3)
        self.rig_begin = [int(v) for v in rig_begin]
        self.n_rigs = len(self.rig_begin) - 1
        self.pts, self.nrm, self.angles = pts, nrm, np.asarray(angles, F64).reshape(120, 2)
        self.scale, self.flags, self.prm = scale, flags, prm or params()
        self.state = np.zeros((self.n_rigs, SLOTS), STATE)

    def reset(self, rig=None):
        if rig is None:
            self.state[:] = 0
        else:
            self.state[rig] = 0

    def step(self, frames, n_heads, heads, n_persons, persons, present=None, fit_prm=None):
        fit_prm = fit_prm or fr.params()
        out = np.zeros((self.n_rigs, SLOTS), RECORD)
        for g in range(self.n_rigs):
            self._rig(g, frames, n_heads, heads, int(n_persons[g]), persons[g], present, fit_prm, out[g])
        return out

    def _rig(self, g, frames, n_heads, heads, n_persons, persons, present, fit_prm, out):
        c0, c1 = self.rig_begin[g], self.rig_begin[g + 1]
        pm = sum(1 << k for k in range(c1 - c0) if present is None or present[c0 + k])
        if pm == 0:
            out["status"] = ABSENT
            return
        prm, st = self.prm, self.state[g]
        slots, ids, founded, freed = bind(st["id"].tolist(), st["tracked"].tolist(), persons, n_persons, n_heads, heads.shape[1])
        for s in range(SLOTS):
            if s in founded or s in freed:
                st[s] = 0
            st[s]["id"] = ids[s]
        for s, slot in enumerate(slots):
            if slot is None:
                continue
            what, i = slot
            e = np.zeros((), STATE) if what == "unbound" else st[s]
            p = persons[i] if i is not None else None
            rec = out[s]
            rec["person"] = NO_PERSON if i is None else i
            free_it = False
            if e["tracked"]:
                views = (int(e["views_used"]) | (int(p["views"]) if p is not None else 0)) & pm
                if views == 0:
                    e["lost"], e["have_prev"] = _sat(e["lost"]), 0
                    rec["id"], rec["status"], rec["age"], rec["lost"] = e["id"], ABSENT, e["age"], e["lost"]
                    if int(e["lost"]) > prm["max_coast"]:
                        st[s] = 0
                    continue
                R = e["R"].copy()
                if (self.flags & MOTION) and e["have_prev"]:
                    with np.errstate(all="ignore"):
                        t = (e["t"] + (e["t"] - e["t_prev"])).astype(F32)
                else:
                    t = e["t"].copy()
                sched, carried = (0, prm["iterations_tracked"]), True
            else:
                b = int(p["best_cam"])
                R = detected_rotation(self.Vs[b], heads[b][int(p["best_head"])]["pose"]["rotation"], self.angles)
                t = np.asarray(p["world"], F32).copy()
                views = int(p["views"]) & pm
                sched, carried = (fit_prm["coarse_iterations"], fit_prm["iterations"]), False
            start = np.zeros((), INSTANCE)
            start["first_cam"], start["views"], start["R"], start["t"], start["scale"] = c0, views, R, t, F32(self.scale)
            fp = dict(fit_prm, coarse_iterations=sched[0], iterations=sched[1])
            Rf, tf, r = vr.fit(frames, self.Ks, self.Vs, self.us, c0, views, self.pts, self.nrm, R.reshape(3, 3), t, F32(self.scale), fp)
            why = 0
            if r["status"] != fr.OK:
                why |= BAD_STATUS
            if r["points"] < prm["keep_points"]:
                why |= BAD_POINTS
            if r["sum_r2_fixed"] > int(F64(prm["rms_max"]) * F64(prm["rms_max"]) * F64(1048576.0)) * r["points"]:
                why |= BAD_RMS
            if p is not None:
                with np.errstate(all="ignore"):
                    d = tf.astype(F64) - np.asarray(p["world"], F32).astype(F64)
                    if not (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= F64(prm["max_jump"]) * F64(prm["max_jump"]):
                        why |= BAD_JUMP
            rec["fit"] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"], r["views_used"])
            rec["instance"] = start
            if why == 0:
                e["t_prev"] = e["t"]
                e["R"], e["t"], e["views_used"] = Rf.reshape(9), tf, r["views_used"]
                e["have_prev"] = e["tracked"]
                e["tracked"], e["age"], e["lost"] = 1, _sat(e["age"]), 0
                rec["instance"]["R"], rec["instance"]["t"] = Rf.reshape(9), tf
                rec["status"] = CARRIED if carried else FITTED
            else:
                e["tracked"], e["have_prev"], e["age"] = 0, 0, 0
                e["lost"] = _sat(e["lost"])
                rec["status"] = REJECTED | why
                free_it = p is None
            rec["id"] = p["id"] if what == "unbound" else e["id"]
            rec["age"], rec["lost"] = e["age"], e["lost"]
            if free_it:
                st[s] = 0
