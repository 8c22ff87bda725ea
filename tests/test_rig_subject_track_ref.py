"""Facts of the rule of DESIGN.md section 30 (include/depthhead_hip.h, "following each rig person with its own subject's model") held
on its restatement, tests/rig_subject_track_ref.py, over the splatted rigs of tests/rig_subject_track_scenes.py: binding at the first
accepted step and the subject's model from the next; an unseen bound entry; an unbound person; a stranger's tries and waits; a
rejection; coasts within and beyond max_coast; a slot founded again; a rig with no present camera; the caller's binding; nobody
enrolled.  No GPU.  Run as a program (PYTHONPATH=. python tests/test_rig_subject_track_ref.py) it is the evaluation of section 30 on
rendered frames: some twenty seconds of numpy, which is why no test runs it."""
import math

import numpy as np

import ident_ref as ir
import ident_views_ref as ivr
import rig_fit_track_ref as rf
import rig_subject_track_ref as rs
import rig_subject_track_scenes as sc
import subject_track_scenes as sts

W, H, NAME = 160, 120, "642"
UNKNOWN = rs.UNKNOWN
F, C, R, A = rf.FITTED, rf.CARRIED, rf.REJECTED, rf.ABSENT
# the angle table as the header states it (the library's is the C library's cos and sin of the same arguments)
ANGLES = np.array([[math.cos((i - 60) / 60.0 * 3.14159), math.sin((i - 60) / 60.0 * 3.14159)] for i in range(120)])
# The splatted 160x120 rigs are coarser than rendered frames: over three views a known head's best mean square is 6 to 9 mm^2 and
# the stranger's about 15 (printed by the tests below), so these scenes run with a limit between them -- and with rms_max = 8 mm for
# the tracker, since the generic head fits a coarse frame of another head at a mean square of 15 to 25 mm^2.
IDENT = dict(min_points=16, max_rms=3.4)
RMS_MAX = 8.0


def tracker(rigs, steps, n_subjects=3, enrolled=None, sub=None, prm=None, gone=(), ident=None):
    s = sc.scene(NAME, n_subjects, W, H, tuple(rigs), steps, gone=tuple(gone))
    st = sts.restated_set(NAME, n_subjects)[3]
    tr = rs.Tracker(s.Ks, s.V, s.u, s.rig_begin, st, sts.generic(NAME), ANGLES, prm=rf.params(**dict(dict(rms_max=RMS_MAX), **(prm or {}))),
                    ident_prm=ivr.params(**(ident or IDENT)), sub_prm=sub, enrolled=enrolled)
    return tr, s


def step(tr, s, k, items, present=None):
    return tr.step(s.frames[k], *s.inputs(items), present=present)


def kinds(rec):
    return (rec["track"]["status"] & 0xFF).tolist()


def means(rec):
    return rec["ident"]["sum_r2_best"] / 1048576.0 / np.maximum(rec["ident"]["points_best"], 1)


def test_an_entry_binds_at_its_first_accepted_step_and_is_fitted_with_its_subjects_model_from_the_next():
    tr, s = tracker(((3, (0, 2)), (2, (1,))), 4)
    rec = np.stack([step(tr, s, k, [s.item(k, 0, 0, 7, best=k % 3), s.item(k, 0, 1, 9, best=1), s.item(k, 1, 0, 4)]) for k in range(4)])
    live = rec[:, [0, 0, 1], [0, 1, 0]]
    print(means(live[0]))
    assert kinds(live[0]) == [F] * 3 and all(kinds(r) == [C] * 3 for r in live[1:])
    assert live["identified"].tolist() == [[1, 1, 1]] + [[0, 0, 0]] * 3 and (live["ident"]["status"][0] == ir.OK).all()
    assert (live["model"][0] == UNKNOWN).all() and (live["track"]["instance"]["model"][0] == 3).all()        # the generic model, entry S
    assert all(r["subject"].tolist() == [0, 2, 1] for r in live)
    assert all(r["model"].tolist() == [0, 2, 1] and r["track"]["instance"]["model"].tolist() == [0, 2, 1] for r in live[1:])
    assert (live["ident"]["status"][1:] == ir.SKIPPED).all() and not live["ident"][1:]["best"].any()           # zeros where none ran
    assert tr.state["bound_age"][0, :2].tolist() == [3, 3] and tr.state["bound_age"][1, 0] == 3 and not tr.state["tries"].any()
    # an unused slot: zeros but for the SKIPPED status and the two words that say "nobody"
    idle = rec[3, 1, 5].copy()
    assert (idle["ident"]["status"], idle["subject"], idle["model"]) == (ir.SKIPPED, UNKNOWN, UNKNOWN)
    idle["ident"]["status"], idle["subject"], idle["model"] = 0, 0, 0
    assert not idle.tobytes().strip(b"\0")
    # the bound steps fit better than the generic rig tracker on the same frames (subject 1 of three IS the generic head)
    gen = rf.Tracker(s.Ks, s.V, s.u, s.rig_begin, *sts.generic(NAME), ANGLES, prm=rf.params(rms_max=RMS_MAX))
    grec = np.stack([gen.step(s.frames[k], *s.inputs([s.item(k, 0, 0, 7, best=k % 3), s.item(k, 0, 1, 9, best=1), s.item(k, 1, 0, 4)]))
                     for k in range(4)])[:, [0, 0, 1], [0, 1, 0]]
    assert live["track"]["fit"][0].tobytes() == grec["fit"][0].tobytes() and live["track"][0].tobytes() != grec[0].tobytes()
    own = live["track"]["fit"]["sum_r2_fixed"][1:] / live["track"]["fit"]["points"][1:]
    other = grec["fit"]["sum_r2_fixed"][1:] / grec["fit"]["points"][1:]
    assert (own[:, :2] < other[:, :2]).all() and (own[:, 2] == other[:, 2]).all()


def test_an_unseen_bound_entry_is_still_fitted_with_its_model_and_an_unbound_person_is_never_identified():
    tr, s = tracker(((3, (2, 0)),), 4)
    seq = [[s.item(0, 0, 0, 5), s.item(0, 0, 1, 0)], [s.item(1, 0, 1, 0)], [s.item(2, 0, 1, 0)], [s.item(3, 0, 0, 5), s.item(3, 0, 1, 0)]]
    rec = np.stack([step(tr, s, k, items)[0] for k, items in enumerate(seq)])
    entry, person = rec[:, 0], rec[:, 1]
    assert kinds(entry) == [F, C, C, C] and entry["track"]["person"].tolist() == [0, rf.NO_PERSON, rf.NO_PERSON, 0]
    assert entry["subject"].tolist() == [2] * 4 and entry["model"].tolist() == [UNKNOWN, 2, 2, 2] and tr.state["bound_age"][0, 0] == 3
    # id 0: fitted with the generic model at every step, never identified, nothing carried
    assert kinds(person) == [F] * 4 and (person["track"]["id"] == 0).all() and (person["track"]["instance"]["model"] == 3).all()
    assert not person["identified"].any() and (person["subject"] == UNKNOWN).all() and (person["model"] == UNKNOWN).all() and not person["tries"].any()
    assert not tr.state["fit"]["id"][0, 1:].any() and (tr.state["subject"][0, 1:] == UNKNOWN).all()


def test_a_stranger_is_never_bound_and_its_tries_and_waits_follow_retry_and_max_tries():
    def run(steps, **sub):
        tr, s = tracker(((3, (sc.STRANGER,)),), 8, sub=rs.params(**sub))
        return tr, np.stack([step(tr, s, k, [s.item(k, 0, 0, 7)])[0, 0] for k in range(steps)])
    tr, rec = run(8, retry=2, max_tries=2)
    print(means(rec[:1]))
    assert (rec["subject"] == UNKNOWN).all() and (rec["model"] == UNKNOWN).all()
    assert rec["identified"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]          # wait 2 -> 1 -> 0, the second try, then tries == max_tries
    assert rec["tries"].tolist() == [1, 1, 1, 2, 2, 2, 2, 2] and (rec["ident"]["status"][rec["identified"] == 1] == ir.FAR).all()
    assert tr.state["wait"][0, 0] == 0 and tr.state["tries"][0, 0] == 2
    _, rec = run(4, retry=0, max_tries=0)                                   # no wait and no limit: every accepted step tries
    assert rec["identified"].tolist() == [1, 1, 1, 1] and rec["tries"].tolist() == [1, 2, 3, 4]
    assert run(4, retry=0, max_tries=1)[1]["identified"].tolist() == [1, 0, 0, 0]
    assert run(4, retry=1, max_tries=0)[1]["identified"].tolist() == [1, 0, 1, 0]


def test_a_rejected_seen_entry_unbinds_and_binds_again():
    tr, s = tracker(((3, (1,)),), 5, gone=((2, 0, 0),))
    rec = np.stack([step(tr, s, k, [s.item(k, 0, 0, 7)])[0, 0] for k in range(5)])
    assert kinds(rec) == [F, C, R, F, C] and (rec["track"]["id"] == 7).all()
    assert rec["subject"].tolist() == [1, 1, UNKNOWN, 1, 1] and rec["model"].tolist() == [UNKNOWN, 1, 1, UNKNOWN, 1]
    assert rec["identified"].tolist() == [1, 0, 0, 1, 0] and rec["track"]["instance"]["model"][2] == 1       # the rejected start named the subject
    assert tr.state["bound_age"][0, 0] == 1


def test_a_coast_keeps_the_binding_within_max_coast_and_loses_it_beyond_and_another_id_starts_unbound():
    tr, s = tracker(((3, (2,)),), 8, prm=dict(max_coast=1))
    seen = lambda k, pid=7: [s.item(k, 0, 0, pid, views=0b011, best=k % 2)]
    only2 = [0, 0, 1]
    script = [(seen(0), None), ([], only2), (seen(2), None), ([], only2), ([], only2), (seen(5, 8), None), (seen(6, 8), None)]
    rec = np.stack([step(tr, s, k, items, present)[0, 0] for k, (items, present) in enumerate(script)])
    assert kinds(rec) == [F, A, C, A, A, F, C]
    assert rec["subject"].tolist() == [2, 2, 2, 2, UNKNOWN, 2, 2] and rec["track"]["lost"].tolist() == [0, 1, 0, 1, 2, 0, 0]
    assert rec["model"].tolist() == [UNKNOWN, UNKNOWN, 2, UNKNOWN, UNKNOWN, UNKNOWN, 2] and rec["identified"].tolist() == [1, 0, 0, 0, 0, 1, 0]
    assert rec["track"]["id"].tolist() == [7, 7, 7, 7, 7, 8, 8]          # the freed slot, founded again by another id, started unbound
    assert not rec["track"]["instance"][1].tobytes().strip(b"\0")


def test_a_rig_with_no_present_camera_keeps_everything():
    tr, s = tracker(((2, (0,)), (2, (1,))), 3)
    items = lambda k: [s.item(k, 0, 0, 3), s.item(k, 1, 0, 4)]
    step(tr, s, 0, items(0))
    before = tr.state.copy()
    rec = step(tr, s, 1, items(1), present=[0, 0, 1, 1])
    assert tr.state[0].tobytes() == before[0].tobytes() and tr.state[1].tobytes() != before[1].tobytes()
    assert (rec[0]["track"]["status"] == A).all() and rec[0, 0]["subject"] == 0 and (rec[0, 1:]["subject"] == UNKNOWN).all()
    assert not rec[0]["identified"].any() and (rec[0]["model"] == UNKNOWN).all() and rec[1, 0]["model"] == 1
    rec = step(tr, s, 2, items(2))
    assert kinds(rec[:, 0]) == [C, C] and rec[:, 0]["model"].tolist() == [0, 1]


def test_the_callers_own_binding():
    tr, s = tracker(((3, (0, sc.STRANGER)),), 3)
    items = lambda k: [s.item(k, 0, 0, 5), s.item(k, 0, 1, 6)]
    before = tr.state.copy()
    tr.bind(0, 5, 2)                                                        # before a track exists no entry holds the id: nothing
    assert tr.state.tobytes() == before.tobytes()
    rec0 = step(tr, s, 0, items(0))[0]
    assert rec0["model"][:2].tolist() == [UNKNOWN, UNKNOWN] and rec0["identified"][:2].tolist() == [1, 1]
    assert rec0["subject"][:2].tolist() == [0, UNKNOWN] and rec0["tries"][:2].tolist() == [0, 1]
    tr.bind(0, 6, 1)                                                        # over a stranger that failed a try
    tr.bind(0, 5, None)                                                     # and a release
    tr.bind(0, 99, 2)                                                       # an id nobody holds
    assert tr.state["tries"][0, :2].tolist() == [0, 0] and tr.state["wait"][0, :2].tolist() == [0, 0]
    assert tr.state["subject"][0, :3].tolist() == [UNKNOWN, 1, UNKNOWN]
    rec1 = step(tr, s, 1, items(1))[0]
    assert rec1["model"][:2].tolist() == [UNKNOWN, 1] and rec1["identified"][:2].tolist() == [1, 0] and rec1["subject"][:2].tolist() == [0, 1]
    assert tr.state["bound_age"][0, :2].tolist() == [0, 1]


def test_nobody_enrolled_and_the_mask_replaced():
    tr, s = tracker(((3, (1,)),), 3, enrolled=[0, 0, 0], sub=rs.params(retry=0, max_tries=0))
    rec = step(tr, s, 0, [s.item(0, 0, 0, 7)])[0, 0]
    assert (rec["identified"], rec["ident"]["status"], rec["ident"]["eligible"], rec["subject"], rec["tries"]) == (1, ir.NO_CANDIDATE, 0, UNKNOWN, 1)
    tr.set_enrolled([1, 0, 1])                                              # the true subject is no candidate: FAR or another, never 1
    rec = step(tr, s, 1, [s.item(1, 0, 0, 7)])[0, 0]
    assert rec["identified"] == 1 and rec["ident"]["eligible"] == 2 and rec["subject"] != 1 and rec["ident"]["best"] in (0, 2)
    tr.set_enrolled(None)
    tr.bind(0, 7, None)
    rec = step(tr, s, 2, [s.item(2, 0, 0, 7)])[0, 0]
    assert (rec["identified"], rec["ident"]["status"], rec["subject"]) == (1, ir.OK, 1)


if __name__ == "__main__":
    import rig_subject_track_eval
    rig_subject_track_eval.main()
