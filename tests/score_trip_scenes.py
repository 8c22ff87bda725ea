"""Scenes that send the workgroups of the subject trackers' score kernels on many trips of mixed kinds (test_score_trip_scenes.py on
the CPU, test_gpu_score_trips.py on the GPU; DESIGN.md sections 29, 30 and 32).  k_subject_track_score and k_rig_subject_score run a
fixed grid of G = min(units * S, 2 * compute units) workgroups over the step's pairs (list entry, subject), the subject the fast
index: workgroup b takes the pairs b, b + G, b + 2 G, ... below L * S, where L entries are listed, and stages the subject's model anew
on every trip.  With S = 64 and G = 512 every trip of a workgroup has the same subject; here S is chosen so that G mod S is not 0
and has no factor in common with S, and the mask of enrolled subjects places which trips run and which are skipped.

The trip table (trips) is integer arithmetic on the header's and the DESIGN sections' words, not the kernel's loop.  The want
list's order is free across the waves of the update kernel, so what a case places across waves depends on the subject alone:
enrolled or not, and which model.  Where every wanting unit lies in one update wave -- at most 64 cameras, at most 4 rigs of 16
slots -- and all of them want, a unit's list position is its index, and the kind of a refit (short: FEW_POINTS at the first pass;
full) can be placed too.

Camera tracker: subject_track_scenes.sequence over the gallery "162" (or "lathe31x33", 1 025 points: streamed) of S subjects,
frames of 64 x 48, camera c showing subject (7 c + 3) mod S.  Rig tracker: rig_subject_track_scenes.scene of one-camera rigs, rig g
showing subject (11 g + 5) mod S under sixteen ids on its one head, each id's person record a little further off, so that every
slot of a rig is in use with a start of its own.  A fit of 1 + 2 iterations, an identification of 1, tracker parameters under which
every fit is accepted and identification parameters under which nobody binds (min_ratio 1e6) with retry = 0 and max_tries = 0:
every unit wants at every step.  Every scene and every restated run is computed once and handed out read-only.  No GPU."""
import functools
import math

import numpy as np

import fit_ref as fr
import fit_track_ref as ft
import fit_track_scenes as fts
import ident_ref as ir
import ident_views_ref as ivr
import rig_fit_track_ref as rf
import rig_subject_track_ref as rs
import rig_subject_track_scenes as sc
import subject_track_ref as stf
import subject_track_scenes as sts
import tracker_wave_scenes as tws

NAME, STREAMED = "162", "lathe31x33"          # 162 points are staged in LDS, 1 025 are one more than fit there
W, H, STEPS = tws.W, tws.H, 3
WAVE, SLOTS = tws.WAVE, rs.SLOTS
FIT, TRACK = tws.FIT, tws.TRACK
CANDIDATES = (65, 63, 61, 67)                 # gallery sizes tried in this order
MI355X_GRID = 512                             # 2 * 256 compute units: the grid the CPU tests compute the tables for
FIRST = 2                                     # the lower of the two enrolled subjects
# "never": nobody binds where two candidates or more are eligible (AMBIGUOUS at min_ratio 1e6).  "far": the same with a max_rms no
# mean square reaches (2^-20 mm: a sum of one fixed-point unit over 162 points is above its square), so that one eligible
# candidate alone does not bind either -- every decision is FAR.  "gate": "never" with a gate of GATE mm; see kinds() for the counts
# it gives.  "binds": whoever is best binds (the rig of 34 cameras).
NEVER = dict(min_points=16, max_rms=np.inf, min_ratio=1e6, iterations=1)
GATE = 4.0
IDENT = {"never": NEVER, "gate": dict(NEVER, gate=GATE), "far": dict(NEVER, max_rms=2.0 ** -20), "binds": dict(NEVER, min_ratio=1.0)}
SHORT, FULL, OTHER = 0, 1, 2                  # kinds of a run pair: FEW_POINTS before any step; every iteration taken; anything else


# ---- the trip table
def choose_subjects(G):
    """The first gallery size of CANDIDATES whose step G mod S is not 0 and has no factor in common with S: a workgroup's subject
    then changes on every trip and comes back only after S of them.  (G = 512: S = 65, a step of 57.)"""
    for S in CANDIDATES:
        if G % S != 0 and math.gcd(G % S, S) == 1:
            return S
    raise AssertionError(f"no gallery size of {CANDIDATES} gives a grid of {G} workgroups a changing subject")


def trips(G, S, L):
    """Per workgroup b of G its trips [(entry, subject)] over L listed entries and S subjects: the pairs b + k G below L S, taken
    apart with the subject the fast index.  Closed forms: ceil((L S - b) / G) trips, and the subject moves by G mod S a trip."""
    total, step = L * S, G % S
    out = []
    for b in range(G):
        count = 0 if b >= total else (total - b + G - 1) // G
        out.append([((b + k * G) // S, (b % S + k * step) % S) for k in range(count)])
    return out


def trip_counts(table):
    return sorted({len(t) for t in table})


def subjects_in_a_row(table, enrolled, pattern):
    """How many times a workgroup's consecutive trips show `pattern` -- a string of 'r' (the subject is enrolled: the pair may run)
    and 's' (not enrolled: skipped) -- with all the enrolled subjects among them different."""
    n, hits = len(pattern), 0
    for t in table:
        for i in range(len(t) - n + 1):
            subj = [s for _, s in t[i:i + n]]
            if all((enrolled[s] != 0) == (p == "r") for s, p in zip(subj, pattern)):
                ran = [s for s, p in zip(subj, pattern) if p == "r"]
                hits += len(set(ran)) == len(ran)
    return hits


def mask(S, subjects=None):
    """The enrolled mask [S] as a tuple: 1 for the listed subjects, None: everybody."""
    return tuple(1 if subjects is None or s in subjects else 0 for s in range(S))


def two(G, S, apart):
    """The two enrolled subjects `apart` trips of a workgroup from one another."""
    return FIRST, (FIRST + apart * (G % S)) % S


def one_wave_units(G, S, per_unit, trips_min=3):
    """The fewest units of per_unit list entries each, all in one update wave, whose L S pairs give every workgroup at least trips_min
    trips and are no multiple of G (a partial last round): (units, L)."""
    for units in range(1, WAVE // per_unit + 1):
        L = units * per_unit
        if L * S >= trips_min * G and (L * S) % G != 0:
            return units, L
    raise AssertionError(f"no {trips_min} trips of {G} workgroups within one update wave of {S} subjects")


# ---- the scenes
def cam_who(n, S):
    return tuple((7 * c + 3) % S for c in range(n))


@functools.lru_cache(maxsize=None)
def cam_scene(name, S, n):
    """(frames [STEPS, n, H, W] u16, Ks [n, 3, 3], poses POSE_DTYPE [STEPS, n]); camera c is the same in every n."""
    frames, Ks, _, _, poses = sts.sequence(name, S, W, H, cam_who(n, S), STEPS)
    return frames, Ks, poses


def rig_who(n_rigs, S):
    return tuple((11 * g + 5) % S for g in range(n_rigs))


@functools.lru_cache(maxsize=None)
def rig_scene(name, S, n_rigs):
    """n_rigs rigs of one camera and one person each, STEPS steps; rig g is the same in every n_rigs."""
    return sc.scene(name, S, W, H, tuple((1, (who,)) for who in rig_who(n_rigs, S)), STEPS)


def rig_items(s, k):
    """Sixteen ids on the one head of every rig at step k, id 100 + i's person record 10 + 2 i mm off the truth: the records are
    rounded to whole mm, and 2 mm along a unit vector move one coordinate by more than 1, so no two starts are equal."""
    return [s.item(k, g, 0, 100 + i, offset_mm=10.0 + 2.0 * i) for g in range(s.n_rigs) for i in range(SLOTS)]


@functools.lru_cache(maxsize=None)
def restated_set(name, S):
    return sts.restated_set(name, S)[3]           # (never changed by a tracker)


# ---- the restated runs: tws.Run(records, the state before each step, the state after) over the steps of `masks`
@functools.lru_cache(maxsize=None)
def cam_run(name, S, n, masks, ident="never", angles_key=None):
    """The restated SubjectFitTracker over cam_scene(name, S, n), masks[k] the enrolled mask of step k."""
    frames, Ks, poses = cam_scene(name, S, n)
    tr = stf.Tracker(Ks, restated_set(name, S), sts.generic(name), tws.table(angles_key), prm=ft.params(**TRACK),
                     ident_prm=ir.params(**IDENT[ident]), sub_prm=stf.params(0, 0), enrolled=masks[0])
    sup, rec, placed, state = fts.good_support(n), [], [], []
    for k, m in enumerate(masks):
        tr.set_enrolled(m)
        placed.append(tr.state.copy())
        rec.append(tr.step(frames[k], poses[k], sup, None, fr.params(**FIT)))
        state.append(tr.state.copy())
    return tws.Run(*tws.frozen(rec, placed, state))


@functools.lru_cache(maxsize=None)
def rig_run(name, S, n_rigs, masks, ident="never", angles_key=None):
    """The restated RigSubjectFitTracker over rig_scene(name, S, n_rigs) with rig_items, masks[k] the enrolled mask of step k."""
    s = rig_scene(name, S, n_rigs)
    tr = rs.Tracker(s.Ks, s.V, s.u, s.rig_begin, restated_set(name, S), sts.generic(name), tws.table(angles_key), prm=rf.params(**TRACK),
                    ident_prm=ivr.params(**IDENT[ident]), sub_prm=rs.params(0, 0), enrolled=masks[0])
    rec, placed, state = [], [], []
    for k, m in enumerate(masks):
        tr.set_enrolled(m)
        placed.append(tr.state.copy())
        rec.append(tr.step(s.frames[k], *s.inputs(rig_items(s, k)), fit_prm=fr.params(**FIT)))
        state.append(tr.state.copy())
    return tws.Run(*tws.frozen(rec, placed, state))


def run(kind, *args):
    return (cam_run if kind == "camera" else rig_run)(*args)


def entries(kind, units):
    """The list entries of `units` cameras, or of `units` rigs with every slot in use."""
    return units if kind == "camera" else units * SLOTS


def first_units(a_run, n):
    return tws.first_cameras(a_run, n)


# ---- short refits among full ones.  Under IDENT["gate"] a model a few subjects off the head in the frame finds fewer than 16
# points within GATE mm and its refit ends FEW_POINTS before its first step, while the models near the truth run their one
# iteration.  With G = 512 and S = 65, step 0, everybody enrolled (test_score_trip_scenes.py holds these counts):
#   camera tracker, 24 cameras, 1 560 pairs: 852 short and 708 full; a short trip directly before a full one 175 times, the reverse 270;
#   rig tracker, 2 rigs, 32 slots, 2 080 pairs: 978 short and 1 102 full; short before full 191 times, the reverse 492.
# (A gate of 2 mm leaves 33 full pairs of the 1 560, one of 6 mm 252 short ones; at 4 mm the pair of the subject in the frame runs in
# 10 of the 24 cameras and 13 of the 32 slots -- the fit of 1 + 2 iterations it starts from is a coarse one.)
# KIND_COUNTS[kind]: (short, full, short before full, full before short)
KIND_COUNTS = {"camera": (852, 708, 175, 270), "rig": (978, 1102, 191, 492)}


@functools.lru_cache(maxsize=None)
def kinds(kind, S, units, angles_key=None):
    """[entries, S] u8: SHORT, FULL or OTHER per (list entry, subject) of step 0 under IDENT["gate"] with everybody enrolled, from
    ident_ref.score (ident_views_ref.score) on the instances the restated step accepted.  One update wave, everybody wanting: entry
    e is camera e, or slot e % 16 of rig e // 16."""
    prm = ir.params(**IDENT["gate"])
    st = restated_set(NAME, S)
    rec = run(kind, NAME, S, units, (mask(S),), "gate", angles_key).records[0].reshape(-1)
    assert (rec["identified"] == 1).all() and len(rec) == entries(kind, units) <= WAVE
    out = np.zeros((len(rec), S), np.uint8)
    for e, r in enumerate(rec):
        t = r["track"]["instance"]
        for s in range(S):
            if kind == "camera":
                frames, Ks, _ = cam_scene(NAME, S, units)
                inst = {"frame": e, "R": t["R"].reshape(3, 3), "t": t["t"], "scale": np.float32(t["scale"])}
                got = ir.score(frames[0, e], Ks[e], st.pts[s], st.nrm[s], inst, prm)[2]
            else:
                sn = rig_scene(NAME, S, units)
                inst = {"first_cam": int(t["first_cam"]), "views": int(t["views"]), "R": t["R"].reshape(3, 3), "t": t["t"],
                        "scale": np.float32(t["scale"])}
                got = ivr.score(sn.frames[0], sn.Ks, sn.V, sn.u, st.pts[s], st.nrm[s], inst, prm)[2]
            short = got["status"] == fr.FEW_POINTS and got["steps"] == 0
            full = got["status"] == fr.OK and got["steps"] == prm["iterations"]
            out[e, s] = SHORT if short else FULL if full else OTHER
    out.setflags(write=False)
    return out


def kinds_in_a_row(table, kind_of, first, second):
    """How many times a workgroup's trip of kind `first` comes directly before one of kind `second`."""
    return sum(1 for t in table for (e0, s0), (e1, s1) in zip(t, t[1:]) if kind_of[e0, s0] == first and kind_of[e1, s1] == second)


# ---- the rig of 34 cameras: person 0 (subject 0, id 7) seen by the cameras 0, 31, 32 and 33, person 1 (subject 2, id 8) by camera 33
# alone; three subjects, everybody enrolled, whoever is best binds at step 0 and step 1 is a carried fit with the bound model.
WIDE_CAMS, WIDE_S = 34, 3
WIDE_VIEWS = ((1 << 0) | (1 << 31) | (1 << 32) | (1 << 33), 1 << 33)


@functools.lru_cache(maxsize=None)
def wide_scene():
    return sc.scene(NAME, WIDE_S, W, H, ((WIDE_CAMS, (0, 2)),), 2)


def wide_items(s, k):
    return [s.item(k, 0, 0, 7, views=WIDE_VIEWS[0], best=32), s.item(k, 0, 1, 8, views=WIDE_VIEWS[1], best=33)]


@functools.lru_cache(maxsize=None)
def wide_run(angles_key=None):
    s = wide_scene()
    tr = rs.Tracker(s.Ks, s.V, s.u, s.rig_begin, restated_set(NAME, WIDE_S), sts.generic(NAME), tws.table(angles_key), prm=rf.params(**TRACK),
                    ident_prm=ivr.params(**IDENT["binds"]), sub_prm=rs.params(0, 0))
    rec, placed, state = [], [], []
    for k in range(2):
        placed.append(tr.state.copy())
        rec.append(tr.step(s.frames[k], *s.inputs(wide_items(s, k)), fit_prm=fr.params(**FIT)))
        state.append(tr.state.copy())
    return tws.Run(*tws.frozen(rec, placed, state))
