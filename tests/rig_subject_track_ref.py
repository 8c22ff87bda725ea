"""Following each rig person with its own subject's model (include/depthhead_hip.h, "following each rig person
with its own subject's model") restated in numpy and plain Python, one rig and one slot at a time, written from the header text.  It
composes the restatements of the three sections the rule composes: rig_fit_track_ref's bind and detected rotation and its slot
step (steps 2 - 6 of section 22, here with the points and normals of the slot's model: the bound subject's as the restated set
holds them now, or the generic ones), section 29's binding lifecycle on the four words beside each entry, and for a slot that wants
it section 28's identification (ident_views_ref.why_not and score, ident_ref.decide) of the slot's accepted instance over the
step's frames.  test_rig_subject_track_ref.py holds it to scenes whose answer is known; test_gpu_rig_subject_tracker.py holds the GPU
to it byte for byte."""
import numpy as np

import fit_ref as fr
import ident_ref as ir
import ident_views_ref as ivr
import rig_fit_track_ref as rf
import subject_track_ref as stf
import view_fit_ref as vr
from rig_fit_track_ref import ABSENT, BAD_JUMP, BAD_POINTS, BAD_RMS, BAD_STATUS, CARRIED, FITTED, MOTION, NONE, REJECTED, SLOTS  # noqa: F401

F32, F64 = np.float32, np.float64
UNKNOWN = ir.UNKNOWN
U32_MAX = 0xFFFFFFFF
STATE = np.dtype([("fit", rf.STATE), ("subject", "<u4"), ("wait", "<u4"), ("tries", "<u4"), ("bound_age", "<u4")])
RECORD = np.dtype([("track", rf.RECORD), ("ident", ir.RECORD_DTYPE), ("subject", "<u4"), ("model", "<u4"), ("identified", "<u4"),
                   ("tries", "<u4")])
assert STATE.itemsize == 104 and RECORD.itemsize == 184

params = stf.params                  # (retry, max_tries): section 29's


def _sat(v):
    return min(int(v) + 1, U32_MAX)


def initial(shape):
    st = np.zeros(shape, STATE)
    st["subject"] = UNKNOWN
    return st


def unbind(e):
    e["subject"], e["wait"], e["tries"], e["bound_age"] = UNKNOWN, 0, 0, 0


def lifecycle(e, accepted, max_tries):
    """Rule 2 on the entry step 1 left (a freed entry is zeros: not tracked).  True: the entry wants identification."""
    if not e["fit"]["tracked"]:
        unbind(e)
        return False
    if not accepted:
        return False
    if int(e["subject"]) != UNKNOWN:
        e["bound_age"] = _sat(e["bound_age"])
        return False
    if int(e["wait"]) == 0 and (max_tries == 0 or int(e["tries"]) < max_tries):
        return True
    if int(e["wait"]) > 0:
        e["wait"] = int(e["wait"]) - 1
    return False


class Tracker:
    """The state of every rig and the step over all of them.  st: the restated set (subjects_ref.Set or surface_ref.Set), read as
    it stands at each step; generic: (points, normals)."""

    def __init__(self, Ks, Vs, us, rig_begin, st, generic, angles, scale=1.0, flags=0, prm=None, ident_prm=None, sub_prm=None, enrolled=None):
        self.Ks = np.asarray(Ks, F32).reshape(-1, 3, 3)
        self.Vs, self.us = np.asarray(Vs, F32).reshape(-1, 3, 3), np.asarray(us, F32).reshape(-1, 3)
        self.rig_begin = [int(v) for v in rig_begin]
        self.n_rigs = len(self.rig_begin) - 1
        self.st, self.generic, self.angles = st, generic, np.asarray(angles, F64).reshape(120, 2)
        self.scale, self.flags = scale, flags
        self.prm, self.ident_prm, self.sub_prm = prm or rf.params(), ident_prm or ivr.params(), sub_prm or params()
        self.set_enrolled(enrolled)
        self.state = initial((self.n_rigs, SLOTS))

    def reset(self, rig=None):
        if rig is None:
            self.state[:] = initial((self.n_rigs, SLOTS))
        else:
            self.state[rig] = initial(SLOTS)

    def bind(self, rig, rig_id, subject):
        """The caller's binding of the entry of `rig` that holds rig_id (None: nothing happens); subject None unbinds."""
        for e in self.state[rig]:
            if int(e["fit"]["id"]) == int(rig_id) != 0:
                e["subject"] = UNKNOWN if subject is None else int(subject)
                e["wait"], e["tries"], e["bound_age"] = 0, 0, 0
                return

    def set_enrolled(self, enrolled):
        self.enrolled = None if enrolled is None else [int(e) for e in enrolled]

    def step(self, frames, n_heads, heads, n_persons, persons, present=None, fit_prm=None):
        fit_prm = fit_prm or fr.params()
        out = np.zeros((self.n_rigs, SLOTS), RECORD)
        out["ident"]["status"] = ir.SKIPPED
        out["model"] = UNKNOWN
        for g in range(self.n_rigs):
            self._rig(g, frames, n_heads, heads, int(n_persons[g]), persons[g], present, fit_prm, out[g])
            out[g]["subject"], out[g]["tries"] = self.state[g]["subject"], self.state[g]["tries"]
        return out

    def _rig(self, g, frames, n_heads, heads, n_persons, persons, present, fit_prm, out):
        c0, c1 = self.rig_begin[g], self.rig_begin[g + 1]
        pm = sum(1 << k for k in range(c1 - c0) if present is None or present[c0 + k])
        if pm == 0:                                                   # step 0: the state, bindings included, is kept
            out["track"]["status"] = ABSENT
            return
        S = len(self.st)
        st = self.state[g]
        # ---- section 22's bind; every entry it founds or frees starts from zeros and unbound
        slots, ids, founded, freed = rf.bind(st["fit"]["id"].tolist(), st["fit"]["tracked"].tolist(), persons, n_persons, n_heads, heads.shape[1])
        for s in range(SLOTS):
            if s in founded or s in freed:
                st[s] = initial(1)[0]
            st[s]["fit"]["id"] = ids[s]
        for s, slot in enumerate(slots):
            if slot is None:
                continue
            what, i = slot
            e = initial(1)[0] if what == "unbound" else st[s]
            bound = what != "unbound" and int(e["subject"]) < S
            model = int(e["subject"]) if bound else S
            pts, nrm = (self.st.pts[model], self.st.nrm[model]) if bound else self.generic
            accepted, fitted, free_it = self._slot(e["fit"], c0, pm, frames, heads, persons[i] if i is not None else None, i, what, model, pts, nrm,
                                          fit_prm, out[s]["track"])
            if fitted and bound:
                out[s]["model"] = model
            if what == "unbound":
                continue                                              # nothing of it is carried, and it is never identified
            if free_it:
                st[s] = initial(1)[0]                                 # freed: zeros, and the four words with them
                continue
            if lifecycle(e, accepted, self.sub_prm["max_tries"]):
                self._identify(e, frames, out[s])

    def _slot(self, e, c0, pm, frames, heads, p, i, what, model, pts, nrm, fit_prm, rec):
        """Steps 2 - 6 of section 22 for one slot on the entry's first 88 bytes `e` (zeros for an unbound person), with the model's
        points and normals.  Returns (accepted, whether a fit ran, whether the entry is freed: the caller zeroes it)."""
        prm = self.prm
        rec["person"] = rf.NO_PERSON if i is None else i
        if e["tracked"]:
            views = (int(e["views_used"]) | (int(p["views"]) if p is not None else 0)) & pm
            if views == 0:
                e["lost"], e["have_prev"] = _sat(e["lost"]), 0
                rec["id"], rec["status"], rec["age"], rec["lost"] = e["id"], ABSENT, e["age"], e["lost"]
                return False, False, int(e["lost"]) > prm["max_coast"]
            R = e["R"].copy()
            if (self.flags & MOTION) and e["have_prev"]:
                with np.errstate(all="ignore"):
                    t = (e["t"] + (e["t"] - e["t_prev"])).astype(F32)
            else:
                t = e["t"].copy()
            sched, carried = (0, prm["iterations_tracked"]), True
        else:
            b = int(p["best_cam"])
            R = rf.detected_rotation(self.Vs[b], heads[b][int(p["best_head"])]["pose"]["rotation"], self.angles)
            t = np.asarray(p["world"], F32).copy()
            views = int(p["views"]) & pm
            sched, carried = (fit_prm["coarse_iterations"], fit_prm["iterations"]), False
        start = np.zeros((), rf.INSTANCE)
        start["first_cam"], start["model"], start["views"], start["R"], start["t"], start["scale"] = c0, model, views, R, t, F32(self.scale)
        fp = dict(fit_prm, coarse_iterations=sched[0], iterations=sched[1])
        Rf, tf, r = vr.fit(frames, self.Ks, self.Vs, self.us, c0, views, pts, nrm, R.reshape(3, 3), t, F32(self.scale), fp)
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
        rec["id"] = p["id"] if what == "unbound" else e["id"]
        rec["age"], rec["lost"] = e["age"], e["lost"]
        return why == 0, True, why != 0 and p is None             # (an unseen entry is freed after a rejection)

    def _identify(self, e, frames, rec):
        """Rule 3: section 28's identification of the slot's accepted instance, and what it makes of the four words."""
        S, ident = len(self.st), rec["ident"]
        t = rec["track"]["instance"]
        inst = {"first_cam": int(t["first_cam"]), "views": int(t["views"]), "R": t["R"].reshape(3, 3).copy(), "t": t["t"].copy(),
                "scale": F32(t["scale"])}
        ident["best"] = ident["second"] = UNKNOWN
        status = ir.SKIPPED
        if ivr.why_not(inst, 0, len(frames), 1, fr.OK, self.st.pts.shape[1], self.st.radius, ir.largest(self.st)) is None:
            row = [None] * S
            for s in range(S):
                if self.enrolled is None or self.enrolled[s]:
                    row[s] = ivr.score(frames, self.Ks, self.Vs, self.us, self.st.pts[s], self.st.nrm[s], inst, self.ident_prm)[2]
            status, best, second, eligible = ir.decide(row, self.ident_prm)
            ident["eligible"] = eligible
            if best is not None:
                ident["best"], ident["points_best"], ident["sum_r2_best"] = best, row[best]["points"], row[best]["sum_r2_fixed"]
            if second is not None:
                ident["second"], ident["points_second"], ident["sum_r2_second"] = second, row[second]["points"], row[second]["sum_r2_fixed"]
        ident["status"] = status
        if status == ir.OK:
            e["subject"], e["bound_age"] = int(ident["best"]), 0
        else:
            e["tries"], e["wait"] = _sat(e["tries"]), self.sub_prm["retry"]
        rec["identified"] = 1
