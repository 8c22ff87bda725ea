"""Scenes that put more than one wave of cameras in front of the fit trackers' per-camera kernels (test_tracker_wave_scenes.py on
the CPU, test_gpu_tracker_waves.py on the GPU; DESIGN.md sections 19 and 29).  k_fit_track_seed / _update and k_subject_track_seed /
_update run one lane per camera in workgroups of one wave of 64 lanes, and k_subject_track_update builds the step's compact want
list from a ballot, one atomic per wave and a rank within the wave; so the scenes have up to 130 cameras -- waves of 64, 64 and 2
lanes -- and scripts that place which cameras want identification at each step.  Built on subject_track_scenes.sequence: gallery
"162" of three subjects, frames of 64 x 48, camera c showing the stranger where c % 5 == 0 and subject c % 3 elsewhere; a fit of 1 + 2
iterations and tracker parameters under which every fit of a head is accepted.  Every restated run is computed once (the
restatement is the cost: about 0.5 s a step at 130 cameras) and handed out read-only.  The rule is per camera, so the run of the
first n cameras IS the first n columns of the run of all 130 (first_cameras; the CPU test holds one fresh run to it).  No GPU."""
import collections
import functools
import math

import numpy as np

import fit_ref as fr
import fit_track_ref as ft
import fit_track_scenes as fts
import ident_ref as ir
import subject_track_ref as stf
import subject_track_scenes as sts

NAME, S, W, H, N, STEPS, WAVE = "162", 3, 64, 48, 130, 6, 64
# the angle table as the header states it (the library's is the C library's cos and sin of the same arguments)
ANGLES = np.array([[math.cos((i - 60) / 60.0 * 3.14159), math.sin((i - 60) / 60.0 * 3.14159)] for i in range(120)])
FIT = dict(coarse_iterations=1, iterations=2)
TRACK = dict(rms_max=4096.0, keep_points=1, max_jump=4096.0)              # every fit of a head is accepted
ALWAYS_BINDS = dict(min_points=16, max_rms=np.inf, min_ratio=1.0)         # every identification ends DH_IDENT_OK
NEVER_BINDS = dict(ALWAYS_BINDS, min_ratio=1e6)                           # with S > 1 every one ends DH_IDENT_AMBIGUOUS
IDENT = {"always": ALWAYS_BINDS, "never": NEVER_BINDS}

# A restated run: records [steps, n], the state as the calls before each step left it [steps, n], the state after each step [steps, n]
Run = collections.namedtuple("Run", "records placed state")


def who(n=N):
    return tuple(sts.STRANGER if c % 5 == 0 else c % 3 for c in range(n))


@functools.lru_cache(maxsize=None)
def scene(gone=()):
    """(frames [STEPS, N, H, W] u16, Ks [N, 3, 3], poses POSE_DTYPE [STEPS, N]); gone: (step, camera) pairs whose frame is empty."""
    frames, Ks, _, _, poses = sts.sequence(NAME, S, W, H, who(), STEPS, gone=tuple(gone))
    return frames, Ks, poses


def table(angles_key=None):
    """The angle table of a run's key: None is the header's, else the bytes of another [120, 2] f64 (the library's own)."""
    return ANGLES if angles_key is None else np.frombuffer(angles_key, np.float64).reshape(120, 2)


def angles_key(angles):
    """The key of a table: None where it is the header's, so that a run restated for the CPU test serves the GPU tests too."""
    return None if np.asarray(angles).tobytes() == ANGLES.tobytes() else np.asarray(angles, np.float64).tobytes()


def tracker(n, ident, angles_key=None, retry=0, max_tries=0):
    """A fresh restated subject tracker over the first n cameras."""
    return stf.Tracker(scene()[1][:n], sts.restated_set(NAME, S)[3], sts.generic(NAME), table(angles_key), prm=ft.params(**TRACK),
                       ident_prm=ir.params(**IDENT[ident]), sub_prm=stf.params(retry, max_tries))


def frozen(*arrays):
    out = tuple(np.stack(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def first_cameras(run, n):
    return Run(*(a[:, :n] for a in run))


class Replay:
    """A restated run served again through the restated tracker's step(): each call hands out the next step's records and
    leaves the state that step left.  placed(k) is the state after the calls (bind, reset) that precede step k."""

    def __init__(self, run):
        self.run, self.k, self.state = run, 0, run.placed[0]

    def placed(self, k):
        assert k == self.k
        self.state = self.run.placed[k]

    def step(self, frames, poses, support, present=None, fit_prm=None):
        k, self.k = self.k, self.k + 1
        self.state = self.run.state[k]
        return self.run.records[k]


# ---- the want script: which cameras are unbound from outside before each step.  After step 0 every camera is bound and accepted, a
# bound camera never wants, an unbound one whose wait is 0 does: the cameras unbound before a step are the step's want list.
UNBINDS = ((), tuple(range(64, 128)), (0, 63, 129), (), tuple(range(0, N, 2)))
WANT_PER_WAVE = ((64, 64, 2), (0, 64, 0), (2, 0, 1), (0, 0, 0), (32, 32, 1))


def unbinds(k, n=N):
    return tuple(c for c in UNBINDS[k] if c < n)


def wanting(k, n=N):
    """identified [n] of step k of the want script."""
    return [1] * n if k == 0 else [int(c in UNBINDS[k]) for c in range(n)]


def per_wave(identified):
    return tuple(int(np.sum(identified[w:w + WAVE])) for w in range(0, len(identified), WAVE))


@functools.lru_cache(maxsize=None)
def want_run(angles_key=None, n=N, steps=len(UNBINDS)):
    """The want script under ALWAYS_BINDS with retry = 0 and max_tries = 0."""
    frames, _, poses = scene()
    tr, sup = tracker(n, "always", angles_key), fts.good_support(n)
    rec, placed, state = [], [], []
    for k in range(steps):
        for c in unbinds(k, n):
            tr.bind(c, None)
        placed.append(tr.state.copy())
        rec.append(tr.step(frames[k, :n], poses[k, :n], sup, None, fr.params(**FIT)))
        state.append(tr.state.copy())
    return Run(*frozen(rec, placed, state))


@functools.lru_cache(maxsize=None)
def never_run(angles_key=None, n=65, steps=3, retry=0, max_tries=0):
    """No call between the steps, under NEVER_BINDS: with retry = 0 and max_tries = 0 every camera wants at every step."""
    frames, _, poses = scene()
    tr, sup = tracker(n, "never", angles_key, retry, max_tries), fts.good_support(n)
    rec, placed, state = [], [], []
    for k in range(steps):
        placed.append(tr.state.copy())
        rec.append(tr.step(frames[k, :n], poses[k, :n], sup, None, fr.params(**FIT)))
        state.append(tr.state.copy())
    return Run(*frozen(rec, placed, state))


# ---- the binding lifecycle under NEVER_BINDS: every step's fit is accepted and every identification fails, so rule 2 and rule 3
# of the header give each row by hand -- (identified, tries after the step, wait after the step) per step.  A step with wait == 0
# and (max_tries == 0 or tries < max_tries) wants: tries + 1, wait = retry.  Any other step with wait > 0: wait - 1.  Else nothing.
#   (retry 0, max_tries 1): step 0 wants (tries 0 < 1) -> tries 1, wait 0; from step 1 on wait is 0 but tries 1 < 1 fails, and wait is not
#                           above 0: nothing changes.
#   (1, 2): step 0 wants -> (1, 1, 1); step 1 wait 1 -> 0; step 2 wait 0 and tries 1 < 2: wants -> (1, 2, 1); step 3 wait 1 -> 0; steps 4
#           and 5 wait 0 but tries 2 < 2 fails: nothing.
#   (2, 0): no limit.  Step 0 wants -> wait 2; steps 1, 2 count it down; step 3 wants -> tries 2, wait 2; steps 4, 5 count down.
#   (0, 2): max_tries on the compare: tries 0 < 2 and 1 < 2 want at steps 0 and 1 (wait stays 0), 2 < 2 fails from step 2 on.
LIFECYCLE = {
    (0, 1): [(1, 1, 0)] + [(0, 1, 0)] * 5,
    (1, 2): [(1, 1, 1), (0, 1, 0), (1, 2, 1), (0, 2, 0), (0, 2, 0), (0, 2, 0)],
    (2, 0): [(1, 1, 2), (0, 1, 1), (0, 1, 0), (1, 2, 2), (0, 2, 1), (0, 2, 0)],
    (0, 2): [(1, 1, 0), (1, 2, 0)] + [(0, 2, 0)] * 4,
}
LIFECYCLE_CAMERAS = 4


def lifecycle_run(retry, max_tries, angles_key=None):
    return never_run(angles_key, LIFECYCLE_CAMERAS, STEPS, retry, max_tries)


def lifecycle(records, state, c):
    """[(identified, tries, wait)] per step of camera c, from records [steps, n] and the states after the steps [steps, n]."""
    return [(int(records["identified"][k, c]), int(records["tries"][k, c]), int(state["wait"][k, c])) for k in range(len(records))]


# ---- every start kind on both sides of a wave boundary, arranged after step 0 of an ALWAYS_BINDS tracker (every camera tracked and
# bound).  Six kinds do not fit on the two cameras either side of 63 | 64, so the neighbours carry the rest.
CARRIED_BOUND, CARRIED_UNBOUND, DETECTED_UNBOUND, DETECTED_BOUND, ABSENT, NO_TRACK = range(6)
START_KINDS = {58: ABSENT, 59: NO_TRACK, 60: CARRIED_BOUND, 61: DETECTED_UNBOUND, 62: CARRIED_UNBOUND, 63: DETECTED_BOUND,
               64: DETECTED_UNBOUND, 65: CARRIED_BOUND, 66: NO_TRACK, 67: ABSENT, 68: DETECTED_BOUND, 69: CARRIED_UNBOUND,
               122: DETECTED_BOUND, 123: CARRIED_BOUND, 124: NO_TRACK, 125: CARRIED_UNBOUND, 126: DETECTED_UNBOUND, 127: ABSENT,
               128: NO_TRACK, 129: CARRIED_UNBOUND}
# per start kind: (the track status, identified) of the step
START_ANSWER = {CARRIED_BOUND: (ft.CARRIED, 0), CARRIED_UNBOUND: (ft.CARRIED, 1), DETECTED_UNBOUND: (ft.FITTED, 1),
                DETECTED_BOUND: (ft.FITTED, 0), ABSENT: (ft.ABSENT, 0), NO_TRACK: (ft.NONE, 0)}


def callers_subject(c):
    return (c + 1) % S


def arrange_start_kinds(tr):
    """The calls on `tr` (the GPU's tracker or the restated one) that place START_KINDS; -> (present [N] u8, support [N]) of step 1."""
    present, sup = np.ones(N, np.uint8), fts.good_support(N)
    for c, kind in START_KINDS.items():
        if kind in (DETECTED_UNBOUND, DETECTED_BOUND, NO_TRACK):
            tr.reset(c)
        if kind == CARRIED_UNBOUND:
            tr.bind(c, None)
        elif kind == DETECTED_BOUND:
            tr.bind(c, callers_subject(c))
        elif kind == ABSENT:
            present[c] = 0
        elif kind == NO_TRACK:
            sup["mass"][c] = 0
    return present, sup


@functools.lru_cache(maxsize=None)
def start_kinds_run(angles_key=None):
    frames, _, poses = scene()
    tr = tracker(N, "always", angles_key)
    first = tr.state.copy()
    rec0 = tr.step(frames[0], poses[0], fts.good_support(N), None, fr.params(**FIT))
    after0 = tr.state.copy()
    present, sup = arrange_start_kinds(tr)
    placed = tr.state.copy()
    rec1 = tr.step(frames[1], poses[1], sup, present, fr.params(**FIT))
    return Run(*frozen([rec0, rec1], [first, placed], [after0, tr.state.copy()]))


# ---- the plain fit tracker over three steps: per camera a plan that names its kinds at steps 0, 1, 2.  Step 1 shows ABSENT, NONE,
# FITTED, CARRIED and REJECTED on both sides of 63 | 64 and below 127 | 128; the two cameras above 127 | 128 cannot show five kinds
# in one step and show them over the three: 128 FITTED, CARRIED, REJECTED and 129 NONE, FITTED, ABSENT.
FIT_STEPS = 3
PLANS = {"carried": (ft.FITTED, ft.CARRIED, ft.CARRIED), "absent": (ft.FITTED, ft.ABSENT, ft.CARRIED), "none": (ft.NONE, ft.NONE, ft.FITTED),
         "fitted": (ft.NONE, ft.FITTED, ft.CARRIED), "rejected": (ft.FITTED, ft.REJECTED, ft.FITTED),
         "rejected late": (ft.FITTED, ft.CARRIED, ft.REJECTED), "fitted, absent": (ft.NONE, ft.FITTED, ft.ABSENT)}
FIT_PLAN = {59: "absent", 60: "fitted", 61: "carried", 62: "rejected", 63: "none", 64: "rejected", 65: "none", 66: "absent", 67: "fitted",
            68: "carried", 123: "fitted", 124: "absent", 125: "carried", 126: "none", 127: "rejected", 128: "rejected late", 129: "fitted, absent"}


def fit_kinds(n=N):
    """kinds [FIT_STEPS][n] the plans come to."""
    return [[PLANS[FIT_PLAN.get(c, "carried")][k] for c in range(n)] for k in range(FIT_STEPS)]


@functools.lru_cache(maxsize=None)
def fit_scene():
    """(frames [FIT_STEPS, N, H, W], Ks, poses [FIT_STEPS, N], support [FIT_STEPS, N], present [FIT_STEPS, N]) of FIT_PLAN: a REJECTED
    step is an empty frame, a NONE step a detection without mass, an ABSENT step a present byte of 0."""
    kinds = fit_kinds()
    frames, Ks, poses = scene(tuple((k, c) for k in range(FIT_STEPS) for c in range(N) if kinds[k][c] == ft.REJECTED))
    sup = np.stack([fts.good_support(N) for _ in range(FIT_STEPS)])
    present = np.ones((FIT_STEPS, N), np.uint8)
    for k in range(FIT_STEPS):
        for c in range(N):
            if kinds[k][c] == ft.NONE:
                sup["mass"][k, c] = 0
            elif kinds[k][c] == ft.ABSENT:
                present[k, c] = 0
    for a in (sup, present):
        a.setflags(write=False)
    return frames[:FIT_STEPS], Ks, poses[:FIT_STEPS], sup, present


@functools.lru_cache(maxsize=None)
def fit_run(angles_key=None):
    """The restated fit tracker with the generic model over fit_scene: Run(records, the state before each step, the state after)."""
    frames, Ks, poses, sup, present = fit_scene()
    tr = ft.Tracker(Ks, *sts.generic(NAME), table(angles_key), prm=ft.params(**TRACK))
    rec, placed, state = [], [], []
    for k in range(FIT_STEPS):
        placed.append(tr.state.copy())
        rec.append(tr.step(frames[k], poses[k], sup[k], present[k], fr.params(**FIT)))
        state.append(tr.state.copy())
    return Run(*frozen(rec, placed, state))
