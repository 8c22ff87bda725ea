"""The restatement of multi-view identification (tests/ident_views_ref.py) held to scenes whose answer is
known, on the CPU: with one view and the identity table it is ident_ref.identify field for field; the true subject wins from two
and from three views; an instance that fails a test of taking part is SKIPPED with its pose copied through; and the evaluation --
three subjects enrolled from the middle camera's frames, twelve probes of them and four of a stranger identified over three
views -- gives the counts the shipped default max_rms promises, which is the rule's value."""
import numpy as np
import pytest

import fit_ref as fr
import ident_ref as ir
import ident_views_ref as ivr
import ident_views_scenes as ivs

SMALL = dict(min_points=16, max_rms=np.inf)
FIRST24 = ["points", "steps", "status", "reserved", "sum_r2_fixed"]


def same_pose(a, b):
    return all(np.asarray(a[k], np.float32).tobytes() == np.asarray(b[k], np.float32).tobytes() for k in ("R", "t", "scale"))


def test_one_view_with_the_identity_table_is_the_single_view_call_field_for_field():
    v, t, B, frames, K, inst, frames4, Ks, V, u, world, st = ivs.single_view_twin("162", 3, 96, 96, [0, 2, 1])
    for prm_kw, enrolled, status in ((SMALL, None, None), (dict(SMALL, iterations=0), [1, 0, 1], None), (dict(min_points=16, max_rms=0.5), None, [0, 1, 0])):
        want = ir.identify(frames, K, st, inst, None, enrolled, status, ir.params(**prm_kw))
        got = ivr.identify(frames4, Ks, V, u, st, world, None, None, enrolled, status, ivr.params(**prm_kw))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (got[1], want[1])
        for name in FIRST24:
            assert (got[3][name] == want[3][name]).all(), name
        ran = want[3]["points"] > 0
        assert (got[3]["views_used"][ran] == 1).all() and (got[3]["views_used"][~ran] == 0).all()
        for a, b, w in zip(got[2], want[2], world):
            assert same_pose(a, b) and a["first_cam"] == w["first_cam"] and a["views"] == 1
    assert want[1]["status"][1] == ir.SKIPPED and (want[1]["status"][[0, 2]] != ir.SKIPPED).all()


@pytest.mark.parametrize("masks", [[0b011, 0b110, 0b101], [0b111] * 3])
def test_the_true_subject_wins_from_two_and_from_three_views(masks):
    v, t, B, frames, Ks, V, u, inst, st = ivs.gallery("162", 3, 96, 96, [2, 0, 1], masks=masks, z=400.0)
    subjects, rec, poses, scores = ivr.identify(frames, Ks, V, u, st, inst, ivs.sets_of(inst), prm=ivr.params(**SMALL))
    assert subjects.tolist() == [2, 0, 1] and (rec["status"] == ivr.OK).all() and (rec["eligible"] == 3).all()
    assert scores["views_used"].tolist() == [[m] * 3 for m in masks] and (scores["steps"] > 0).all()
    for p, s in zip(poses, inst):
        assert not same_pose(p, s) and (p["first_cam"], p["views"]) == (s["first_cam"], s["views"])
    # every candidate of an instance is scored over one mask: a one-view mask gives fewer pairs than the two-view one
    fewer = ivr.identify(frames, Ks, V, u, st, [dict(inst[0], views=0b010)], prm=ivr.params(**SMALL))
    assert fewer[0].tolist() == [2] and (fewer[3]["points"] < scores["points"][0]).all()


def test_instances_in_different_sets_and_a_first_camera_that_is_not_0():
    v, t, B, frames, Ks, V, u, inst, st = ivs.gallery("162", 3, 96, 96, [1, 2, 0], sets=[2, 0, 1, 0], masks=[0b11, 0b11, 0b1, 0b10], first_cam=1, z=400.0)
    subjects, rec, _, scores = ivr.identify(frames, Ks, V, u, st, inst, ivs.sets_of(inst), prm=ivr.params(**SMALL))
    assert subjects.tolist() == [0, 1, 2, 1] and (scores["views_used"][:, 0] == [0b11, 0b11, 0b1, 0b10]).all()
    none = ivr.identify(frames, Ks, V, u, st, inst, None, prm=ivr.params(**SMALL))      # sets NULL: all in set 0, which is subject 1's
    assert none[1][[1, 3]].tobytes() == rec[[1, 3]].tobytes() and none[3][[0, 2]].tobytes() != scores[[0, 2]].tobytes()
    assert 0 not in none[1]["best"].tolist() and 2 not in none[0].tolist()


def test_each_test_of_taking_part_skips_with_the_pose_copied_through():
    v, t, B, frames, Ks, V, u, inst, st = ivs.gallery("162", 2, 96, 96, [0, 1])
    good = inst[0]
    bad = [dict(good, views=0), dict(good, views=0b1000), dict(good, first_cam=2, views=0b11), dict(good), dict(good),
           dict(good, t=np.array([np.nan, 0, 0], np.float32)), dict(good, R=(good["R"] * np.float32(1.02)).astype(np.float32)),
           dict(good, scale=np.float32(40.0)), dict(good, R=(good["R"] * np.float32(1.005)).astype(np.float32))]
    sets = [0, 0, 0, 2, 0, 0, 0, 0, 0]
    status = [fr.OK] * 4 + [fr.FEW_POINTS] + [fr.OK] * 4
    big = ir.largest(st)
    assert [ivr.why_not(b, s, 3, 2, f, len(v), st.radius, big) for b, s, f in zip(bad, sets, status)] == [1, 2, 2, 3, 4, 5, 5, 5, None]
    # the order: a later failure does not hide an earlier one
    worst = dict(good, views=0, R=good["R"] * np.float32(np.nan))
    assert ivr.why_not(worst, 9, 3, 2, fr.SINGULAR, 1 << 20, st.radius, big) == 1
    assert ivr.why_not(dict(worst, views=0b1000), 9, 3, 2, fr.SINGULAR, 1 << 20, st.radius, big) == 2
    assert ivr.why_not(dict(worst, views=0b1), 9, 3, 2, fr.SINGULAR, 1 << 20, st.radius, big) == 3
    assert ivr.why_not(dict(worst, views=0b1), 1, 3, 2, fr.SINGULAR, 1 << 20, st.radius, big) == 4
    assert ivr.why_not(dict(worst, views=0b1), 1, 3, 2, None, 1 << 20, st.radius, big) == 5
    assert ivr.why_not(dict(good, views=0b1), 1, 3, 2, None, 1 << 20, st.radius, big) == 6
    assert ivr.why_not(dict(good, views=0b11), 1, 3, 2, None, 16384, st.radius, big) is None       # exactly 32768 terms
    assert ivr.why_not(dict(good, views=0b11), 1, 3, 2, None, 16385, st.radius, big) == 6
    subjects, rec, poses, scores = ivr.identify(frames, Ks, V, u, st, bad, sets, None, None, status, ivr.params(**SMALL))
    assert rec["status"].tolist() == [ivr.SKIPPED] * 8 + [ivr.OK]
    for i in range(8):
        assert subjects[i] == ivr.UNKNOWN and rec["best"][i] == ivr.UNKNOWN and rec["eligible"][i] == 0
        assert not scores[i].tobytes().strip(b"\0")
        assert all(np.asarray(poses[i][k]).tobytes() == np.asarray(bad[i][k]).tobytes() for k in ("R", "t", "scale", "views", "first_cam"))
    assert subjects[8] == 0


def test_nobody_enrolled_and_a_mask():
    v, t, B, frames, Ks, V, u, inst, st = ivs.gallery("162", 3, 96, 96, [1, 2])
    subjects, rec, poses, scores = ivr.identify(frames, Ks, V, u, st, inst, ivs.sets_of(inst), enrolled=[0, 0, 0], prm=ivr.params(**SMALL))
    assert (rec["status"] == ivr.NO_CANDIDATE).all() and (subjects == ivr.UNKNOWN).all() and not scores.tobytes().strip(b"\0")
    assert all(same_pose(p, s) for p, s in zip(poses, inst))
    subjects, rec, _, scores = ivr.identify(frames, Ks, V, u, st, inst, ivs.sets_of(inst), enrolled=[1, 0, 1], prm=ivr.params(**SMALL))
    assert rec["best"].tolist() == [2, 2] and (rec["eligible"] == 2).all() and not scores[:, 1].tobytes().strip(b"\0")   # 1 is no candidate: 2 is nearer than 0


def _bests(views, min_points):
    _, rec, _, _ = ivs.evaluation_result(views, np.inf, min_points)
    truth = ivs.evaluation()[5]
    ms = [None if r["best"] == ir.UNKNOWN else float(ir.mean_square(r["sum_r2_best"], r["points_best"])) for r in rec]
    return rec, truth, ms


def test_the_evaluation_under_the_shipped_default_and_the_default_is_the_rules_value():
    """Three views, the shipped defaults: 12 of 12 known probes named, 4 of 4 stranger probes DH_IDENT_FAR; the default is the
    square root of the geometric mean of the largest known best and the smallest stranger best, to 0.01 mm."""
    subjects, rec, _, frecs = ivs.evaluation_result()
    truth = ivs.evaluation()[5]
    assert all(r["status"] == fr.OK for r in frecs)
    assert subjects.tolist() == [ivr.UNKNOWN if who is None else who for who in truth]
    assert rec["status"].tolist() == [ivr.FAR if who is None else ivr.OK for who in truth]
    assert (rec["points_best"] >= 138).all() and (rec["eligible"] == 3).all()
    rec, truth, ms = _bests(ivs.ALL, 64)
    assert [r["best"] for r, who in zip(rec, truth) if who is not None] == [who for who in truth if who is not None]
    known, stranger = max(m for m, who in zip(ms, truth) if who is not None), min(m for m, who in zip(ms, truth) if who is None)
    assert stranger > known, (known, stranger)                                     # the sets separate
    rule = np.sqrt(np.sqrt(known * stranger))
    assert abs(ivr.DEFAULT_MAX_RMS - rule) <= 0.01, (known, stranger, rule)
    assert (round(known, 4), round(stranger, 4)) == (4.0152, 10.9989)              # the numbers beside the default in the header
    from depthhead_amd import _lib
    assert _lib.IDENT_VIEWS_DEFAULT_MAX_RMS == ivr.DEFAULT_MAX_RMS and ir.DEFAULT_MAX_RMS == 1.68


def test_the_middle_view_alone_decides_nothing_at_the_default_min_points_and_separates_less_at_16():
    rec, truth, _ = _bests(ivs.MIDDLE, 64)
    assert (rec["status"] == ivr.NO_CANDIDATE).all()                               # the best candidate associates 59 .. 66 points of a known head (min_points 16 shows them), 43 .. 50 of the stranger's: no pair stays at or above 64 through its refit
    rec, truth, ms = _bests(ivs.MIDDLE, 16)
    assert [r["best"] for r, who in zip(rec, truth) if who is not None] == [who for who in truth if who is not None]
    known, stranger = max(m for m, who in zip(ms, truth) if who is not None), min(m for m, who in zip(ms, truth) if who is None)
    _, _, ms3 = _bests(ivs.ALL, 16)
    known3, stranger3 = max(m for m, who in zip(ms3, truth) if who is not None), min(m for m, who in zip(ms3, truth) if who is None)
    assert stranger3 / known3 > stranger / known > 1.0, (known, stranger, known3, stranger3)


if __name__ == "__main__":                                                          # the evaluation's table
    truth = ivs.evaluation()[5]
    print("enrolled coefficients:", np.round(ivs.evaluation()[0].state["coeffs"][:3, :4], 4).tolist())
    for views, name in ((ivs.ALL, "three views"), (ivs.MIDDLE, "the middle view")):
        for min_points in (64, 16):
            _, rec, _, frecs = ivs.evaluation_result(views, np.inf, min_points)
            print(f"{name}, min_points {min_points}")
            for who in (0, 1, 2, None):
                rows = [r for r, w in zip(rec, truth) if w == who]
                fits = [f for f, w in zip(frecs, truth) if w == who]
                ms = [None if r["best"] == ir.UNKNOWN else float(ir.mean_square(r["sum_r2_best"], r["points_best"])) for r in rows]
                m2 = [None if r["second"] == ir.UNKNOWN else float(ir.mean_square(r["sum_r2_second"], r["points_second"])) for r in rows]
                print("  ", "stranger" if who is None else f"subject {who}", "generic fit points", [f["points"] for f in fits], "best", [int(r["best"]) if r["best"] != ir.UNKNOWN else None for r in rows],
                      "points", [int(r["points_best"]) for r in rows], "best m", [None if m is None else round(m, 4) for m in ms],
                      "second / best", [None if a is None or b is None else round(b / a, 2) for a, b in zip(ms, m2)])
            rec, truth, ms = _bests(views, min_points)
            if all(m is not None for m in ms):
                known, stranger = max(m for m, w in zip(ms, truth) if w is not None), min(m for m, w in zip(ms, truth) if w is None)
                print(f"   largest known {known:.4f} mm^2, smallest stranger {stranger:.4f} mm^2, ratio {stranger / known:.2f}, rule {np.sqrt(np.sqrt(known * stranger)):.4f} mm")
