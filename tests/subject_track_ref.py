"""Following each tracked head with its own subject's model (include/depthhead_hip.h, "following each
tracked head with its own subject's model") restated in numpy and plain Python, one camera at a time, written from the header
text: section 19's step (fit_track_ref.step_camera) called with the bound subject's points and normals or with the generic ones,
the binding lifecycle, and for a camera that wants it section 27's identification (ident_ref.takes_part, score and decide) of the
step's accepted instance.  The set is a restated one (subjects_ref.Set or surface_ref.Set): its models are read as they stand at
each step.  test_subject_track_ref.py holds it to scenes whose answer is known; test_gpu_subject_tracker.py holds the GPU to it
byte for byte."""
import numpy as np

import fit_ref as fr
import fit_track_ref as ft
import ident_ref as ir

UNKNOWN = ir.UNKNOWN
U32_MAX = 0xFFFFFFFF
STATE = np.dtype([("fit", ft.STATE), ("subject", "<u4"), ("wait", "<u4"), ("tries", "<u4"), ("bound_age", "<u4")])
RECORD = np.dtype([("track", ft.RECORD), ("ident", ir.RECORD_DTYPE), ("subject", "<u4"), ("model", "<u4"), ("identified", "<u4"),
                   ("tries", "<u4")])
assert STATE.itemsize == 92 and RECORD.itemsize == 160


def params(retry=4, max_tries=4):
    return {"retry": int(retry), "max_tries": int(max_tries)}


def _sat(v):
    return min(int(v) + 1, U32_MAX)


def initial(n):
    st = np.zeros(n, STATE)
    st["subject"] = UNKNOWN
    return st


def step_camera(state, c, frames, Ks, st, generic, enrolled, scale, flags, prm, fit_prm, ident_prm, sub_prm, present, pose, sup, angles):
    """One step of camera c.  `state`: a STATE scalar, changed in place; frames [n, h, w] and Ks [n, 3, 3]: the step's; st: the
    restated set; generic: (points, normals); enrolled: [S] or None.  Returns a RECORD scalar."""
    S = len(st)
    rec = np.zeros((), RECORD)
    bound = int(state["subject"]) < S
    mesh = int(state["subject"]) if bound else S
    pts, nrm = (st.pts[mesh], st.nrm[mesh]) if bound else generic
    # 1. section 19's steps 0 - 6 with the chosen model; the start instance names the mesh
    track = ft.step_camera(state["fit"], c, frames[c], Ks[c], pts, nrm, scale, flags, prm, fit_prm, present, pose, sup, angles)
    kind = int(track["status"]) & 0xFF
    fitted = kind not in (ft.NONE, ft.ABSENT)
    if fitted:
        track["instance"]["mesh"] = mesh
    rec["track"] = track
    rec["model"] = mesh if fitted and bound else UNKNOWN
    # 2. the binding lifecycle
    want = False
    if not state["fit"]["tracked"]:
        state["subject"], state["wait"], state["tries"], state["bound_age"] = UNKNOWN, 0, 0, 0
    elif kind in (ft.FITTED, ft.CARRIED):
        if bound:
            state["bound_age"] = _sat(state["bound_age"])
        elif int(state["wait"]) == 0 and (sub_prm["max_tries"] == 0 or int(state["tries"]) < sub_prm["max_tries"]):
            want = True
        elif int(state["wait"]) > 0:
            state["wait"] = int(state["wait"]) - 1
    # 3. identification of the accepted instance
    rec["ident"]["status"] = ir.SKIPPED
    if want:
        inst = {"frame": c, "R": track["instance"]["R"].reshape(3, 3).copy(), "t": track["instance"]["t"].copy(),
                "scale": np.float32(track["instance"]["scale"])}
        ident = rec["ident"]
        ident["best"] = ident["second"] = UNKNOWN
        status = ir.SKIPPED
        if ir.takes_part(inst, len(frames), fr.OK, st.radius, ir.largest(st)):
            row = [None] * S
            for s in range(S):
                if enrolled is None or enrolled[s]:
                    row[s] = ir.score(frames[c], Ks[c], st.pts[s], st.nrm[s], inst, ident_prm)[2]
            status, best, second, eligible = ir.decide(row, ident_prm)
            ident["eligible"] = eligible
            if best is not None:
                ident["best"], ident["points_best"], ident["sum_r2_best"] = best, row[best]["points"], row[best]["sum_r2_fixed"]
            if second is not None:
                ident["second"], ident["points_second"], ident["sum_r2_second"] = second, row[second]["points"], row[second]["sum_r2_fixed"]
        ident["status"] = status
        if status == ir.OK:
            state["subject"], state["bound_age"] = int(ident["best"]), 0
        else:
            state["tries"], state["wait"] = _sat(state["tries"]), sub_prm["retry"]
        rec["identified"] = 1
    rec["subject"], rec["tries"] = state["subject"], state["tries"]
    return rec


class Tracker:
    """The state of n cameras and the step over all of them."""

    def __init__(self, Ks, st, generic, angles, scale=1.0, flags=0, prm=None, ident_prm=None, sub_prm=None, enrolled=None):
        self.Ks = np.asarray(Ks, np.float32).reshape(-1, 3, 3)
        self.n = len(self.Ks)
        self.st, self.generic, self.angles = st, generic, np.asarray(angles, np.float64).reshape(120, 2)
        self.scale, self.flags = scale, flags
        self.prm, self.ident_prm, self.sub_prm = prm or ft.params(), ident_prm or ir.params(), sub_prm or params()
        self.enrolled = None if enrolled is None else [int(e) for e in enrolled]
        self.state = initial(self.n)

    def reset(self, camera=None):
        if camera is None:
            self.state[:] = initial(self.n)
        else:
            self.state[camera] = initial(1)[0]

    def bind(self, camera, subject):
        s = self.state[camera]
        s["subject"] = UNKNOWN if subject is None else int(subject)
        s["wait"], s["tries"], s["bound_age"] = 0, 0, 0

    def set_enrolled(self, enrolled):
        self.enrolled = None if enrolled is None else [int(e) for e in enrolled]

    def step(self, frames, poses, support, present=None, fit_prm=None):
        fit_prm = fit_prm or fr.params()
        out = np.zeros(self.n, RECORD)
        for c in range(self.n):
            out[c] = step_camera(self.state[c], c, frames, self.Ks, self.st, self.generic, self.enrolled, self.scale, self.flags, self.prm,
                                 fit_prm, self.ident_prm, self.sub_prm, present is None or bool(present[c]), poses[c], support[c], self.angles)
        return out
