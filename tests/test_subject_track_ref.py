"""The subject tracker's rule as tests/subject_track_ref.py restates it, on scenes whose answer is known: a
track binds at its first accepted step and is fitted with its subject's model from the next; a stranger is never bound and its
tries and waits follow retry and max_tries on both sides of each compare; a rejected step unbinds; an absent camera keeps its
binding within max_coast and loses it beyond; the caller's own binding; an unenrolled better match is never chosen; and the
evaluation -- section 27's gallery, each of its people and a stranger moving as fit_track_scenes.sequence moves its head -- under
the shipped defaults.  Run as a program it prints the evaluation's table.  No GPU."""
import functools
import math

import numpy as np

import fit_track_ref as ft
import fit_track_scenes as fts
import ident_ref as ir
import ident_scenes as isc
import subject_track_ref as stf
import subject_track_scenes as sts
import surface_scenes as us

W, H, NAME = 96, 96, "642"
UNKNOWN = stf.UNKNOWN
# the angle table as the header states it (the library's is the C library's cos and sin of the same arguments)
ANGLES = np.array([[math.cos((i - 60) / 60.0 * 3.14159), math.sin((i - 60) / 60.0 * 3.14159)] for i in range(120)])
# The splatted 96x96 scenes are coarser than a rendered frame: a known head's best mean square is about 11 mm^2, the stranger's
# 19 to 36 (printed by the tests below), so these scenes run with a limit between them -- and with rms_max = 8 mm for the tracker,
# since the generic head fits the stranger's coarse frames at a mean square of 25 to 45 mm^2.
IDENT = dict(min_points=16, max_rms=3.8)
RMS_MAX = 8.0


def tracker(who, steps, n_subjects=3, enrolled=None, sub=None, prm=None, gone=(), ident=None):
    frames, Ks, _, _, poses = sts.sequence(NAME, n_subjects, W, H, tuple(who), steps, gone=tuple(gone))
    st = sts.restated_set(NAME, n_subjects)[3]
    tr = stf.Tracker(Ks, st, sts.generic(NAME), ANGLES, prm=prm or ft.params(rms_max=RMS_MAX), ident_prm=ir.params(**(ident or IDENT)), sub_prm=sub, enrolled=enrolled)
    return tr, frames, poses, fts.good_support(len(who))


def run(tr, frames, poses, sup, present=None, steps=None):
    return np.stack([tr.step(frames[k], poses[k], sup, None if present is None else present[k]) for k in range(len(frames) if steps is None else steps)])


def kinds(rec):
    return (rec["track"]["status"] & 0xFF).tolist()


def test_a_track_binds_at_its_first_accepted_step_and_is_fitted_with_its_subjects_model_from_the_next():
    tr, frames, poses, sup = tracker((0, 2, 1), 4)
    rec = run(tr, frames, poses, sup)
    print(rec["ident"]["sum_r2_best"][0] / 1048576.0 / rec["ident"]["points_best"][0])
    assert kinds(rec[0]) == [ft.FITTED] * 3 and all(kinds(r) == [ft.CARRIED] * 3 for r in rec[1:])
    assert rec["identified"].tolist() == [[1, 1, 1]] + [[0, 0, 0]] * 3 and (rec["ident"]["status"][0] == ir.OK).all()
    assert (rec["model"][0] == UNKNOWN).all() and (rec["track"]["instance"]["mesh"][0] == 3).all()          # the generic model, entry S
    assert all(r["subject"].tolist() == [0, 2, 1] for r in rec)
    assert all(r["model"].tolist() == [0, 2, 1] and r["track"]["instance"]["mesh"].tolist() == [0, 2, 1] for r in rec[1:])
    assert (rec["ident"]["status"][1:] == ir.SKIPPED).all() and not rec["ident"][1:]["best"].any()          # zeros where none ran
    assert tr.state["bound_age"].tolist() == [3, 3, 3] and tr.state["tries"].tolist() == [0, 0, 0]
    # the bound steps fit better than the generic tracker on the same frames
    gen = ft.Tracker(tr.Ks, *sts.generic(NAME), ANGLES)
    grec = np.stack([gen.step(frames[k], poses[k], sup) for k in range(4)])
    assert rec["track"][0].tobytes() != grec[0].tobytes() and rec["track"]["fit"][0].tobytes() == grec["fit"][0].tobytes()
    own = rec["track"]["fit"]["sum_r2_fixed"][1:] / rec["track"]["fit"]["points"][1:]
    other = grec["fit"]["sum_r2_fixed"][1:] / grec["fit"]["points"][1:]
    assert (own[:, :2] < other[:, :2]).all() and (own[:, 2] == other[:, 2]).all()       # (subject 1 of three IS the generic head: coefficient 0)


def test_a_stranger_is_never_bound_and_its_tries_and_waits_follow_retry_and_max_tries():
    tr, frames, poses, sup = tracker((sts.STRANGER,), 8, sub=stf.params(retry=2, max_tries=2))
    rec = run(tr, frames, poses, sup)[:, 0]
    print(rec["ident"]["sum_r2_best"][0] / 1048576.0 / rec["ident"]["points_best"][0])
    assert (rec["subject"] == UNKNOWN).all() and (rec["model"] == UNKNOWN).all()
    assert rec["identified"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]          # wait 2 -> 1 -> 0, the second try, then tries == max_tries
    assert rec["tries"].tolist() == [1, 1, 1, 2, 2, 2, 2, 2] and (rec["ident"]["status"][rec["identified"] == 1] == ir.FAR).all()
    assert tr.state["wait"][0] == 0 and tr.state["tries"][0] == 2
    # retry = 0 and no limit: every accepted step tries; max_tries = 1: one try
    tr, frames, poses, sup = tracker((sts.STRANGER,), 4, sub=stf.params(retry=0, max_tries=0))
    rec = run(tr, frames, poses, sup)[:, 0]
    assert rec["identified"].tolist() == [1, 1, 1, 1] and rec["tries"].tolist() == [1, 2, 3, 4]
    tr, frames, poses, sup = tracker((sts.STRANGER,), 4, sub=stf.params(retry=0, max_tries=1))
    assert run(tr, frames, poses, sup)[:, 0]["identified"].tolist() == [1, 0, 0, 0]
    tr, frames, poses, sup = tracker((sts.STRANGER,), 4, sub=stf.params(retry=1, max_tries=0))
    assert run(tr, frames, poses, sup)[:, 0]["identified"].tolist() == [1, 0, 1, 0]


def test_a_rejected_step_unbinds_and_the_track_binds_again():
    tr, frames, poses, sup = tracker((1,), 5, gone=((2, 0),))
    rec = run(tr, frames, poses, sup)[:, 0]
    assert kinds(rec) == [ft.FITTED, ft.CARRIED, ft.REJECTED, ft.FITTED, ft.CARRIED]
    assert rec["subject"].tolist() == [1, 1, UNKNOWN, 1, 1] and rec["model"].tolist() == [UNKNOWN, 1, 1, UNKNOWN, 1]
    assert rec["identified"].tolist() == [1, 0, 0, 1, 0] and rec["track"]["instance"]["mesh"][2] == 1          # the rejected start named the subject
    assert tr.state["bound_age"][0] == 1


def test_an_absent_camera_keeps_its_binding_within_max_coast_and_loses_it_beyond():
    present = np.ones((7, 1), np.uint8)
    present[1] = 0; present[3:5] = 0
    tr, frames, poses, sup = tracker((2,), 7, prm=ft.params(rms_max=RMS_MAX, max_coast=1))
    rec = run(tr, frames, poses, sup, present)[:, 0]
    assert kinds(rec) == [ft.FITTED, ft.ABSENT, ft.CARRIED, ft.ABSENT, ft.ABSENT, ft.FITTED, ft.CARRIED]
    assert rec["subject"].tolist() == [2, 2, 2, 2, UNKNOWN, 2, 2]
    assert rec["model"].tolist() == [UNKNOWN, UNKNOWN, 2, UNKNOWN, UNKNOWN, UNKNOWN, 2] and rec["identified"].tolist() == [1, 0, 0, 0, 0, 1, 0]
    assert not rec["track"]["instance"][1].tobytes().strip(b"\0")


def test_the_callers_own_binding():
    tr, frames, poses, sup = tracker((0, 0, sts.STRANGER), 3)
    tr.bind(1, 2)                                                           # before the track starts: the first fit uses subject 2's model
    rec0 = tr.step(frames[0], poses[0], sup)
    assert rec0["model"].tolist() == [UNKNOWN, 2, UNKNOWN] and rec0["identified"].tolist() == [1, 0, 1] and rec0["subject"].tolist() == [0, 2, UNKNOWN]
    tr.bind(2, 1); tr.bind(0, None)
    assert tr.state["tries"][2] == 0 and tr.state["wait"][2] == 0
    rec1 = tr.step(frames[1], poses[1], sup)
    assert rec1["model"].tolist() == [UNKNOWN, 2, 1] and rec1["identified"].tolist() == [1, 0, 0] and rec1["subject"].tolist() == [0, 2, 1]
    assert tr.state["bound_age"].tolist() == [0, 2, 1]


def test_an_unenrolled_better_match_is_never_chosen():
    tr, frames, poses, sup = tracker((1, 1), 2, enrolled=[1, 0, 1], ident=dict(min_points=16, max_rms=np.inf))
    rec = run(tr, frames, poses, sup)
    assert 1 not in rec["subject"].tolist()[0] and 1 not in rec["ident"]["best"][0].tolist() and (rec["ident"]["eligible"][0] == 2).all()
    free = tracker((1, 1), 1, ident=dict(min_points=16, max_rms=np.inf))
    assert run(*free)[0]["subject"].tolist() == [1, 1]
    tr.set_enrolled([0, 0, 0]); tr.reset()
    rec = run(tr, frames, poses, sup, steps=1)
    assert (rec["ident"]["status"] == ir.NO_CANDIDATE).all() and (rec["subject"] == UNKNOWN).all() and rec["tries"].tolist() == [[1, 1]]


# ---- the evaluation
EVAL_SALTS = (0, 1, 2, 3)            # salt 0 is the table's; the others give the margins


@functools.lru_cache(maxsize=None)
def evaluation(salt=0):
    """Per person of section 27's gallery (three enrolled, the stranger last) a list of per-step rows
    (generic status, generic mean square, generic position error mm, generic rotation error deg, the same four of the new rule,
    model, identified, ident status, best, best mean square, subject after the step)."""
    st, enrolled, K, _, _, _ = isc.evaluation()
    v, _, n, _ = us.eval_generic()
    out = []
    for seed in isc.EVAL_SEEDS + (isc.EVAL_STRANGER,):
        frames, K, pos, Rs, poses = sts.eval_sequence(seed, salt=salt)
        tr = stf.Tracker(K[None], st, (v, n), ANGLES, enrolled=enrolled)
        gen = ft.Tracker(K[None], v, n, ANGLES)
        rows = []
        for k in range(len(frames)):
            rec = tr.step(frames[k][None], poses[k:k + 1], fts.good_support(1))[0]
            g = gen.step(frames[k][None], poses[k:k + 1], fts.good_support(1))[0]

            def four(r):
                ms = float(ir.mean_square(r["fit"]["sum_r2_fixed"], r["fit"]["points"])) if r["fit"]["points"] else np.nan
                Rf = r["instance"]["R"].reshape(3, 3).astype(np.float64)
                cos = np.clip((np.trace(Rf @ Rs[k].T) - 1.0) / 2.0, -1.0, 1.0)
                return int(r["status"]), ms, float(np.linalg.norm(r["instance"]["t"].astype(np.float64) - pos[k])), float(np.degrees(np.arccos(cos)))
            idn = rec["ident"]
            mb = float(ir.mean_square(idn["sum_r2_best"], idn["points_best"])) if idn["points_best"] else np.nan
            rows.append(four(g) + four(rec["track"]) + (int(rec["model"]), int(rec["identified"]), int(idn["status"]), int(idn["best"]), mb, int(rec["subject"])))
        out.append(rows)
    return out


def summary(salt):
    """(largest best mean square of a known try, smallest of a stranger try, worst bound-step mean square, worst bound-step
    position error, worst bound-step rotation error) of one salt."""
    ev = evaluation(salt)
    known = max(r[12] for rows in ev[:3] for r in rows if r[9])
    stranger = min(r[12] for r in ev[3] if r[9])
    bound = [r for rows in ev[:3] for r in rows if r[8] != UNKNOWN]
    return known, stranger, max(r[5] for r in bound), max(r[6] for r in bound), max(r[7] for r in bound)


def test_the_evaluation_under_the_shipped_defaults():
    """Measured with this file (its table is DESIGN.md section 29's): every enrolled person binds to themself at step 0 -- the
    first accepted step -- and is fitted with their own model from step 1; the stranger is identified at steps 0 and 5 (retry =
    4), DH_IDENT_FAR both times, and never bound.  Section 27's default max_rms separates the two sets on moving frames: over
    salts 0 - 3 the largest best mean square of a known try is 1.896 mm^2 and the smallest of a stranger's 3.423 mm^2, either side
    of 1.68^2 = 2.822.  The bounds on the bound steps take section 19's margin: twice the worst case over the other salts."""
    ev = evaluation(0)
    for who, rows in enumerate(ev[:3]):
        assert [r[9] for r in rows] == [1] + [0] * (len(rows) - 1), rows
        assert rows[0][10] == ir.OK and all(r[13] == who for r in rows) and all(r[8] == who for r in rows[1:]) and rows[0][8] == UNKNOWN
        assert all(r[4] in (ft.FITTED, ft.CARRIED) for r in rows)
    stranger = ev[3]
    assert [r[9] for r in stranger] == [1, 0, 0, 0, 0, 1, 0, 0] and all(r[13] == UNKNOWN and r[8] == UNKNOWN for r in stranger)
    assert all(r[10] == ir.FAR for r in stranger if r[9])
    others = [summary(s) for s in EVAL_SALTS[1:]]
    known, far, ms, err, rot = summary(0)
    assert max([known] + [o[0] for o in others]) < ir.DEFAULT_MAX_RMS ** 2 < min([far] + [o[1] for o in others])
    assert ms <= 2.0 * max(o[2] for o in others) and err <= 2.0 * max(o[3] for o in others) and rot <= 2.0 * max(o[4] for o in others)
    # what the feature is for: bound steps fit with a smaller mean square than the generic tracker's on the same frames
    gen = np.mean([r[1] for rows in ev[:3] for r in rows[1:]])
    own = np.mean([r[5] for rows in ev[:3] for r in rows[1:]])
    assert own < gen, (own, gen)


if __name__ == "__main__":
    names = {ir.OK: "OK", ir.SKIPPED: "-", ir.NO_CANDIDATE: "NO_CANDIDATE", ir.FAR: "FAR", ir.AMBIGUOUS: "AMBIGUOUS"}
    ev = evaluation(0)
    print("person step | generic: ms mm^2  pos mm  rot deg | subject tracker: model  ms mm^2  pos mm  rot deg | ident  best  m_best  bound")
    for who, rows in enumerate(ev):
        for k, r in enumerate(rows):
            model = "gen" if r[8] == UNKNOWN else str(r[8])
            bound = "-" if r[13] == UNKNOWN else str(r[13])
            best = "-" if not r[9] else str(r[11])
            mb = "-" if not r[9] else f"{r[12]:.3f}"
            print(f"{'stranger' if who == 3 else who!s:8} {k:3d} | {r[1]:7.3f} {r[2]:7.2f} {r[3]:7.2f} | {model:>5} {r[5]:7.3f} {r[6]:7.2f} {r[7]:7.2f} | "
                  f"{names[r[10]]:5} {best:>4} {mb:>7} {bound:>5}")
    carried = [r for rows in ev[:3] for r in rows[1:]]
    print("carried steps of the enrolled, means: generic ms %.3f pos %.2f rot %.2f | own model ms %.3f pos %.2f rot %.2f" %
          tuple(np.mean([r[i] for r in carried]) for i in (1, 2, 3, 5, 6, 7)))
    for s in EVAL_SALTS:
        print("salt %d: largest known m_best %.4f, smallest stranger m_best %.4f, worst bound step ms %.3f pos %.2f mm rot %.2f deg" % ((s,) + summary(s)))
