"""The multi-view shape step's restatement (tests/shape_views_ref.py) on scenes whose answer is known
(tests/shape_views_scenes.py): section 20's subject, the generic head stretched by (1.08, 0.93, 1.06), seen by three cameras on an
arc (-35, 0, +35 degrees) at four sets, 160x120, noise 2, holes 0.02.  No GPU.

Fixed cases hold the rule to its definition.  Measured cases hold alternation over the rig (shape_views_ref.adapt_views) to
DESIGN.md section 23's table and set it beside section 20's alternation (shape_ref.adapt) on the yaw-0 camera's four frames
alone, from the same starts: `python tests/test_shape_views_ref.py` prints that table for seeds 0 .. 11; the tests assert, on the
four OTHER seeds 12 .. 15, twice the table's worst case per figure (the rule of sections 18 to 20), that adapting lowers the
residual rms on every seed, and -- because the table shows it for seeds 0 .. 11 -- that three views leave a smaller mean error
of the z stretch than one."""
import functools
import sys

import numpy as np
import pytest

import fit_ref as fr
import shape_ref as sr
import shape_scenes as ss
import shape_views_ref as svr
import shape_views_scenes as sv
import view_fit_ref as vr
from depthhead_amd import fit, synth

TABLE_SEEDS, TEST_SEEDS = range(0, 12), (12, 13, 14, 15)
C_TRUE = np.array(sv.C_TRUE)
# the worst case of seeds 0 .. 11, three views: rms after (mm), position error after (mm), |c - c_true|
WORST_RMS, WORST_POS, WORST_C = 1.844, 3.92, (0.0169, 0.0186, 0.0480, 0.0318)
# the mean |c_z - 0.06| of seeds 0 .. 11: three views 0.0406, the yaw-0 camera alone 0.0483
EYE, ZERO = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)


def _true(seed, c_true=sv.C_TRUE, n_sets=4):
    frames, Ks, V, u, pos, Rs = sv.subject(seed, n_sets, c_true=c_true)
    return frames, Ks, V, u, sv.true_instances(pos, Rs)


def test_the_identity_view_is_the_single_view_step():
    """One view, V = I, u = 0, one set: every byte of the record is shape_ref.shape_step's on the same poses."""
    v, _, n, B = ss.generic()
    frames, K, pos, Rs = ss.subject(160, 120, 0)
    single = ss.true_instances(pos, Rs) + ss.rough_instances(0, pos, Rs)
    for s in single:
        want = sr.shape_step(frames, K, v, n, B, [s])[0]
        world = [{"first_cam": 0, "views": 1, "R": s["R"], "t": s["t"], "scale": s["scale"]}]
        got = svr.shape_step(frames[s["frame"]][None, None], K[None], EYE, ZERO, v, n, B, world)[0]
        assert got.tobytes() == want.tobytes() and got["points"] > 0
    # all eight frames as eight sets of the one camera, against the one call
    world = [{"first_cam": 0, "views": 1, "R": s["R"], "t": s["t"], "scale": s["scale"]} for s in single[:8]]
    got = svr.shape_step(frames[:, None], K[None], EYE, ZERO, v, n, B, world, sets=range(8))[0]
    assert got.tobytes() == sr.shape_step(frames, K, v, n, B, single[:8])[0].tobytes() and got["instances"] == 8


@pytest.mark.parametrize("seed", (0, 1))
def test_one_step_at_the_true_poses_points_toward_the_subject(seed):
    v, _, n, B = ss.generic()
    frames, Ks, V, u, inst = _true(seed)
    rec = svr.shape_step(frames, Ks, V, u, v, n, B, inst, sets=range(4))[0]
    assert rec["status"] == svr.OK and rec["instances"] == 12 and rec["points"] >= 64
    for k in range(3):                                   # (the nose's true coefficient is 0: it has no sign)
        assert np.sign(rec["delta"][k]) == np.sign(sv.C_TRUE[k]), (k, rec["delta"])
    assert (rec["delta"][4:] == 0.0).all()


# the largest |increment| per field of one step at the true poses with the subject EQUAL to the model, seeds 0 .. 7
STILL_WORST = (0.0083, 0.0103, 0.0057, 0.0463)


@pytest.mark.parametrize("seed", (12, 13))
def test_the_subject_equal_to_the_model_moves_little(seed):
    """What is left when there is nothing to recover is the pixel grid (the depth is read at a pixel, up to half a pixel beside
    the model point's ray).  Reasoning alone bounds it by half a pixel at the largest depth against the head's smallest semi-axis,
    0.062, which is as large as the smallest stretch looked for and so separates nothing; the bound here is measured instead, by
    the project's convention: seeds 0 .. 7 move the three stretches by at most 0.0083, 0.0103 and 0.0057 and the nose field by
    0.0463, and seeds 12 and 13 are held to twice that.  Twice the worst stretch, 0.021, is a third of the smallest true
    stretch (0.06): a step that invented a stretch from nothing would fail here."""
    v, _, n, B = ss.generic()
    frames, Ks, V, u, inst = _true(seed, c_true=(0.0, 0.0, 0.0, 0.0))
    rec = svr.shape_step(frames, Ks, V, u, v, n, B, inst, sets=range(4))[0]
    print("increments", rec["delta"][:4], "bounds", [2.0 * w for w in STILL_WORST])
    assert rec["status"] == svr.OK
    for k in range(4):
        assert abs(rec["delta"][k]) <= 2.0 * STILL_WORST[k], (k, rec["delta"])
    assert 2.0 * max(STILL_WORST[:3]) < min(abs(c) for c in sv.C_TRUE[:3]) / 2.0


def test_an_empty_view_beside_two_that_see_the_head_is_not_a_pair():
    v, _, n, B = ss.generic()
    frames, Ks, V, u, inst = _true(0)
    blind = frames.copy()
    blind[:, 2] = 0
    rec = svr.shape_step(blind, Ks, V, u, v, n, B, inst, sets=range(4))[0]
    two = svr.shape_step(frames, Ks, V, u, v, n, B, [dict(s, views=0b011) for s in inst], sets=range(4))[0]
    assert rec["instances"] == 8 and rec.tobytes() == two.tobytes()
    none = svr.shape_step(np.zeros_like(frames), Ks, V, u, v, n, B, inst, sets=range(4))[0]
    assert (none["status"], none["points"], none["instances"], none["sum_r2_fixed"]) == (svr.FEW_POINTS, 0, 0, 0) and (none["delta"] == 0.0).all()


def test_two_sets_named_in_mixed_order_are_two_calls_summed():
    """points, instances and e of a call over sets (1, 0, 1, 0) are the sums of a call on set 0 and one on set 1."""
    v, _, n, B = ss.generic()
    frames, Ks, V, u, inst = _true(1, n_sets=2)
    four = [inst[1], inst[0], dict(inst[1], views=0b101), dict(inst[0], views=0b010)]
    both = svr.shape_step(frames, Ks, V, u, v, n, B, four, sets=[1, 0, 1, 0])[0]
    a = svr.shape_step(frames[:1], Ks, V, u, v, n, B, [four[1], four[3]])[0]
    b = svr.shape_step(frames[1:], Ks, V, u, v, n, B, [four[0], four[2]])[0]
    for f in ("points", "instances", "sum_r2_fixed"):
        assert int(both[f]) == int(a[f]) + int(b[f]), f
    assert both["instances"] == 9                         # 3 + 3 + 2 + 1 pairs
    # and the order of the instances is free
    again = svr.shape_step(frames, Ks, V, u, v, n, B, four[::-1], sets=[0, 1, 0, 1])[0]
    assert again.tobytes() == both.tobytes()


def test_two_subjects_in_one_call_are_two_calls():
    v, _, n, B = ss.generic()
    fa, Ks, V, u, ia = _true(0, n_sets=2)
    fb, _, _, _, ib = _true(1, n_sets=2)
    frames = np.concatenate([fa, fb])
    both = svr.shape_step(frames, Ks, V, u, v, n, B, ia + ib, sets=[0, 1, 2, 3], subjects=[1, 1, 0, 0], n_subjects=2)
    assert both[1].tobytes() == svr.shape_step(fa, Ks, V, u, v, n, B, ia, sets=[0, 1])[0].tobytes()
    assert both[0].tobytes() == svr.shape_step(fb, Ks, V, u, v, n, B, ib, sets=[0, 1])[0].tobytes()


def test_skipped_instances_change_nothing():
    v, _, n, B = ss.generic()
    frames, Ks, V, u, inst = _true(1)
    some = svr.shape_step(frames, Ks, V, u, v, n, B, inst[:2], sets=[0, 1])[0]
    junk = [dict(s, t=s["t"] + np.float32(40.0)) for s in inst[2:]]
    skipped = svr.shape_step(frames, Ks, V, u, v, n, B, inst[:2] + junk, sets=range(4), subjects=[0, 0, svr.SKIP, svr.SKIP])[0]
    assert some.tobytes() == skipped.tobytes()


def test_few_points_on_either_side_of_min_points():
    v, _, n, B = ss.generic()
    frames, Ks, V, u, inst = _true(0)
    usual = svr.shape_step(frames, Ks, V, u, v, n, B, inst, sets=range(4))[0]
    count = int(usual["points"])
    at = svr.shape_step(frames, Ks, V, u, v, n, B, inst, sets=range(4), prm=svr.params(min_points=count))[0]
    above = svr.shape_step(frames, Ks, V, u, v, n, B, inst, sets=range(4), prm=svr.params(min_points=count + 1))[0]
    assert at.tobytes() == usual.tobytes() and usual["status"] == svr.OK
    assert above["status"] == svr.FEW_POINTS and (above["delta"] == 0.0).all()
    assert (above["points"], above["instances"], above["sum_r2_fixed"]) == (count, 12, usual["sum_r2_fixed"])


def test_two_identical_fields_without_damping_on_either_side_of_the_1e_9_term():
    """lambda = 0 and two identical fields.  Over 12 pairs the diagonal a is about 1e5 and a + 1e-9 is representable, so the
    second pivot is about 2e-9 > 0 and the exit is OK, the two increments sharing the single field's (section 20).  Over 257
    pairs (single views of the four sets, each true pose moved by a few seeded millimetres) the diagonal has outgrown the
    1e-9 term and the multi-view step itself ends SINGULAR, with zero increments and its counts intact."""
    v, _, n, B = ss.generic()
    frames, Ks, V, u, inst = _true(0)
    prm = svr.params(lam=0.0)
    twin_basis = np.stack([B[0], B[0]])
    single = svr.shape_step(frames, Ks, V, u, v, n, B[:1], inst, sets=range(4), prm=prm)[0]
    twin = svr.shape_step(frames, Ks, V, u, v, n, twin_basis, inst, sets=range(4), prm=prm)[0]
    assert single["status"] == svr.OK and twin["status"] == svr.OK
    assert abs((twin["delta"][0] + twin["delta"][1]) - single["delta"][0]) < 1e-6
    jitter = (6.0 * synth.SplitMix(4244).uniform(3 * 257).reshape(257, 3) - 3.0).astype(np.float32)
    many = [dict(inst[i % 4], views=1 << (i // 4 % 3), t=inst[i % 4]["t"] + jitter[i]) for i in range(257)]
    rec = svr.shape_step(frames, Ks, V, u, v, n, twin_basis, many, sets=[i % 4 for i in range(257)], prm=prm)[0]
    assert rec["status"] == svr.SINGULAR and (rec["delta"] == 0.0).all()
    assert rec["instances"] == 257 and rec["points"] > 30 * 257 and rec["sum_r2_fixed"] > 0


# ---------------------------------------------------------------------------------------------------------------- measured
def _after_views(frames, Ks, V, u, v, n, inst, pos):
    """(rms over all views of all sets, the largest position error) after fitting `inst` (set s is instance s) with (v, n)."""
    e = count = 0
    err = []
    for s, it in enumerate(inst):
        _, t, rec = vr.fit(frames[s], Ks, V, u, it["first_cam"], it["views"], v, n, it["R"], it["t"], 1.0)
        e, count = e + rec["sum_r2_fixed"], count + rec["points"]
        err.append(float(np.linalg.norm(t.astype(np.float64) - pos[s])))
    return float(np.sqrt(e / sr.S / count)), max(err)


def _after_single(frames, K, v, n, inst, cam_pos):
    e = count = 0
    err = []
    for s in inst:
        _, t, rec = fr.fit(frames[s["frame"]], K, v, n, s["R"], s["t"], 1.0)
        e, count = e + rec["sum_r2_fixed"], count + rec["points"]
        err.append(float(np.linalg.norm(t.astype(np.float64) - cam_pos[s["frame"]])))
    return float(np.sqrt(e / sr.S / count)), max(err)


@functools.lru_cache(maxsize=None)
def measure(seed):
    """From the same rough world starts: the generic model alone over the rig (rms0, pos0); adapt_views over three views of four
    sets (rms3, pos3, c3); shape_ref.adapt on the yaw-0 camera's four frames alone (rms1, pos1, c1)."""
    v, t, n, B = ss.generic()
    frames, Ks, V, u, pos, Rs = sv.subject(seed)
    starts = sv.rough_instances(seed, pos, Rs)
    rms0, pos0 = _after_views(frames, Ks, V, u, v, n, starts, pos)
    c3, inst3, _ = svr.adapt_views(frames, Ks, V, u, v, t, B, starts, range(len(starts)), fit.vertex_normals)
    va = sr.deform(v, B, c3)
    rms3, pos3 = _after_views(frames, Ks, V, u, va, fit.vertex_normals(va, t), inst3, pos)
    mid = frames[:, sv.MIDDLE]
    cam_pos = [np.asarray(V[sv.MIDDLE], np.float64) @ p + np.asarray(u[sv.MIDDLE], np.float64) for p in pos]
    c1, inst1, _ = sr.adapt(mid, Ks[sv.MIDDLE], v, t, B, sv.single_view(starts, V, u), fit.vertex_normals)
    vb = sr.deform(v, B, c1)
    rms1, pos1 = _after_single(mid, Ks[sv.MIDDLE], vb, fit.vertex_normals(vb, t), inst1, cam_pos)
    return rms0, pos0, rms3, pos3, c3, rms1, pos1, c1


@pytest.mark.parametrize("seed", TEST_SEEDS)
def test_adapt_views_against_the_generic_model(seed):
    """Twice the worst case of seeds 0 .. 11: rms 3.688 mm, position 7.84 mm, |c - c_true| (0.0338, 0.0372, 0.0960, 0.0636).  The z
    stretch is recovered to about a third with three views too (section 23): its bound is what the table gives."""
    rms0, pos0, rms3, pos3, c3, rms1, pos1, c1 = measure(seed)
    err3, err1 = np.abs(c3 - C_TRUE), np.abs(c1 - C_TRUE)
    print(f"seed {seed}: generic rms {rms0:.3f} pos {pos0:.2f}; three views rms {rms3:.3f} pos {pos3:.2f} c {c3} |c - c_true| {err3}; "
          f"one view rms {rms1:.3f} pos {pos1:.2f} c {c1} |c - c_true| {err1}")
    assert rms3 < rms0
    assert rms3 <= 2.0 * WORST_RMS and pos3 <= 2.0 * WORST_POS
    for k in range(4):
        assert err3[k] <= 2.0 * WORST_C[k], (k, err3)


def test_three_views_leave_a_smaller_mean_z_error_than_one():
    """Seeds 0 .. 11 show it (mean |c_z - 0.06| 0.0406 against 0.0483), so seeds 12 .. 15 are held to it: the mean, not each seed."""
    rows = [measure(s) for s in TEST_SEEDS]
    z3 = float(np.mean([abs(r[4][2] - C_TRUE[2]) for r in rows]))
    z1 = float(np.mean([abs(r[7][2] - C_TRUE[2]) for r in rows]))
    print(f"mean |c_z - 0.06| over seeds {TEST_SEEDS}: three views {z3:.4f}, one view {z1:.4f}")
    assert z3 < z1


if __name__ == "__main__":
    rows = [measure(s) for s in TABLE_SEEDS]
    print("| seed | generic rms | generic pos | 3 views: rms | pos | c | abs(c - c_true) | 1 view: rms | pos | c | abs(c - c_true) |")
    for s, (rms0, pos0, rms3, pos3, c3, rms1, pos1, c1) in zip(TABLE_SEEDS, rows):
        print(f"| {s} | {rms0:.3f} | {pos0:.2f} | {rms3:.3f} | {pos3:.2f} | {np.round(c3, 4).tolist()} | {np.round(np.abs(c3 - C_TRUE), 4).tolist()} "
              f"| {rms1:.3f} | {pos1:.2f} | {np.round(c1, 4).tolist()} | {np.round(np.abs(c1 - C_TRUE), 4).tolist()} |")
    e3 = np.array([np.abs(r[4] - C_TRUE) for r in rows])
    e1 = np.array([np.abs(r[7] - C_TRUE) for r in rows])
    print("three views worst: rms", max(r[2] for r in rows), "pos", max(r[3] for r in rows), "c", e3.max(axis=0), "mean", e3.mean(axis=0))
    print("one view    worst: rms", max(r[5] for r in rows), "pos", max(r[6] for r in rows), "c", e1.max(axis=0), "mean", e1.mean(axis=0))
    sys.exit(0)
