"""The shape step's restatement (tests/shape_ref.py) on scenes whose answer is known (tests/shape_scenes.py): a subject whose
head is the generic model stretched by (1.08, 0.93, 1.06), eight seeded poses each, 160x120, noise 2, holes 0.02.  No GPU.

Fixed cases hold the rule to its definition.  Measured cases hold alternation (shape_ref.adapt) to DESIGN.md section 20's table:
`python tests/test_shape_ref.py` prints that table for seeds 0 .. 11; the tests assert, on the four OTHER seeds 12 .. 15, twice
the table's worst case per figure (the rule of sections 18 and 19), and that adapting lowers the residual rms on every seed."""
import sys

import numpy as np
import pytest

import fit_ref as fr
import shape_ref as sr
import shape_scenes as ss
from depthhead_amd import fit

W, H = 160, 120
TABLE_SEEDS, TEST_SEEDS = range(0, 12), (12, 13, 14, 15)
# the worst case of seeds 0 .. 11: rms after (mm), position error after (mm), |c - c_true| per field
WORST_RMS, WORST_POS, WORST_C = 1.918, 17.00, (0.0369, 0.0207, 0.0419, 0.0662)


def _true(seed, c_true=ss.C_TRUE):
    frames, K, pos, Rs = ss.subject(W, H, seed, c_true=c_true)
    return frames, K, ss.true_instances(pos, Rs)


def test_the_pass_is_the_fits():
    """The per-point pass restated here and fit_ref.one_pass give the same e and count, at a true and at a rough pose."""
    v, _, n, _ = ss.generic()
    frames, K, pos, Rs = ss.subject(W, H, 0)
    for s in ss.true_instances(pos, Rs)[:3] + ss.rough_instances(0, pos, Rs)[:3]:
        R, t = s["R"].astype(np.float64), s["t"].astype(np.float64)
        for gate in (25.0, 1.0, 256.0):
            ok, _, res = sr.point_terms(frames[s["frame"]], K, v, n, np.float64(1.0), R, t, gate)
            _, _, e, count = fr.one_pass(frames[s["frame"]], K, v, n, np.float64(1.0), R, t, gate)
            assert (fr._isum(res[ok] * res[ok]), int(ok.sum())) == (e, count)


@pytest.mark.parametrize("seed", (0, 1))
def test_one_step_at_the_true_poses_points_toward_the_subject(seed):
    v, _, n, B = ss.generic()
    frames, K, inst = _true(seed)
    rec = sr.shape_step(frames, K, v, n, B, inst)[0]
    assert rec["status"] == sr.OK and rec["instances"] == 8 and rec["points"] >= 64
    for k in range(3):                                   # (the nose's true coefficient is 0: it has no sign)
        assert np.sign(rec["delta"][k]) == np.sign(ss.C_TRUE[k]), (k, rec["delta"])
    assert (rec["delta"][4:] == 0.0).all()


@pytest.mark.parametrize("seed", (0, 1))
def test_the_subject_equal_to_the_model_moves_little(seed):
    """What is left is the pixel grid: the depth is read at a pixel, up to half a pixel beside the model point's ray.  At the far
    end of the pose range (1200 mm) that is 600 / f mm, and against the smallest semi-axis of the head (75 mm) a relative
    stretch of 8 / f: no increment may reach it."""
    v, _, n, B = ss.generic()
    frames, K, inst = _true(seed, c_true=(0.0, 0.0, 0.0, 0.0))
    rec = sr.shape_step(frames, K, v, n, B, inst)[0]
    bound = 0.5 * 1200.0 / float(K[0, 0]) / 75.0
    print("increments", rec["delta"][:4], "bound", bound)
    assert rec["status"] == sr.OK and (np.abs(rec["delta"][:4]) < bound).all()
    assert bound < min(abs(c) for c in ss.C_TRUE[:3])    # (and that is below every stretch the other tests look for)


def test_an_empty_frame_gives_few_points():
    v, _, n, B = ss.generic()
    frames, K, inst = _true(0)
    rec = sr.shape_step(np.zeros_like(frames), K, v, n, B, inst)[0]
    assert (rec["status"], rec["points"], rec["instances"], rec["sum_r2_fixed"]) == (sr.FEW_POINTS, 0, 0, 0) and (rec["delta"] == 0.0).all()
    rec = sr.shape_step(frames, K, v, n, B, [], n_subjects=2)        # a subject with no instance
    assert (rec["status"] == sr.FEW_POINTS).all() and (rec["points"] == 0).all()


def test_degenerate_bases_go_on_by_the_1e_9_term():
    """lambda = 0.  Two identical fields: A = [[a + 1e-9, a], [a, a + 1e-9]] with a about 1e5, whose second pivot
    (a + 1e-9) - (a / (a + 1e-9)) * a is about 2e-9 > 0 where a + 1e-9 is representable (ulp(1e5) = 1.5e-11): the exit is OK, and
    the two increments share what the single field alone would take.  A field of zeros: its row is 0 but for the pivot 1e-9 > 0,
    its right side 0: the exit is OK, its increment exactly 0 and the other field's the single field's to the bit."""
    v, _, n, B = ss.generic()
    frames, K, inst = _true(0)
    prm = sr.params(lam=0.0)
    single = sr.shape_step(frames, K, v, n, B[:1], inst, prm=prm)[0]
    twin = sr.shape_step(frames, K, v, n, np.stack([B[0], B[0]]), inst, prm=prm)[0]
    assert single["status"] == sr.OK and twin["status"] == sr.OK
    assert abs((twin["delta"][0] + twin["delta"][1]) - single["delta"][0]) < 1e-6 and (twin["delta"][:2] > 0.0).all()
    zero = sr.shape_step(frames, K, v, n, np.stack([B[0], np.zeros_like(B[0])]), inst, prm=prm)[0]
    assert zero["status"] == sr.OK and zero["delta"][1] == 0.0 and zero["delta"][0] == single["delta"][0]
    # and the other exit: a pivot that is not > 0 (a right side and a matrix of NaN never arise from finite sums; a negative one does
    # when the damping is taken away from a zero row)
    assert sr.solve_subject({(0, 0): 0, (0, 1): 0, (1, 1): -1 << 20}, [0, 0], 0, 100, 1, 2, prm)["status"] == sr.SINGULAR


def test_skipped_instances_change_nothing():
    v, _, n, B = ss.generic()
    frames, K, inst = _true(1)
    some = sr.shape_step(frames, K, v, n, B, inst[:5])[0]
    junk = [dict(s, t=s["t"] + np.float32(40.0)) for s in inst[5:]]
    skipped = sr.shape_step(frames, K, v, n, B, inst[:5] + junk, subjects=[0] * 5 + [sr.SKIP] * 3)[0]
    assert some.tobytes() == skipped.tobytes()


def test_two_subjects_in_one_call_are_two_calls():
    v, _, n, B = ss.generic()
    fa, K, ia = _true(0)
    fb, _, ib = _true(1)
    frames = np.concatenate([fa, fb])
    both = sr.shape_step(frames, K, v, n, B, ia + [dict(s, frame=s["frame"] + 8) for s in ib], subjects=[1] * 8 + [0] * 8, n_subjects=2)
    assert both[1].tobytes() == sr.shape_step(fa, K, v, n, B, ia)[0].tobytes()
    assert both[0].tobytes() == sr.shape_step(fb, K, v, n, B, ib)[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------- measured
def _after_fit(frames, K, v, n, inst, pos):
    """(rms over all frames, the largest position error) after fitting `inst` with the model (v, n)."""
    e = count = 0
    err = []
    for s in inst:
        _, t, rec = fr.fit(frames[s["frame"]], K, v, n, s["R"], s["t"], 1.0)
        e, count = e + rec["sum_r2_fixed"], count + rec["points"]
        err.append(float(np.linalg.norm(t.astype(np.float64) - pos[s["frame"]])))
    return float(np.sqrt(e / sr.S / count)), max(err)


def measure(seed):
    """Generic model alone against adapt, from the same rough starts: (rms0, pos0, rms1, pos1, coefficients)."""
    v, t, n, B = ss.generic()
    frames, K, pos, Rs = ss.subject(W, H, seed)
    starts = ss.rough_instances(seed, pos, Rs)
    rms0, pos0 = _after_fit(frames, K, v, n, starts, pos)
    c, inst, _ = sr.adapt(frames, K, v, t, B, starts, fit.vertex_normals)
    va = sr.deform(v, B, c)
    rms1, pos1 = _after_fit(frames, K, va, fit.vertex_normals(va, t), inst, pos)
    return rms0, pos0, rms1, pos1, c


@pytest.mark.parametrize("seed", TEST_SEEDS)
def test_adapt_against_the_generic_model(seed):
    """Twice the worst case of seeds 0 .. 11: rms 3.836 mm, position 34.0 mm, |c - c_true| (0.0738, 0.0414, 0.0838, 0.1324).
    The z stretch is only partly recovered against t.z (section 20): its bound is what the table gives, not the stretch."""
    rms0, pos0, rms1, pos1, c = measure(seed)
    err = np.abs(c - np.array(ss.C_TRUE))
    print(f"seed {seed}: generic rms {rms0:.3f} pos {pos0:.2f}; adapted rms {rms1:.3f} pos {pos1:.2f}; c {c}; |c - c_true| {err}")
    assert rms1 < rms0
    assert rms1 <= 2.0 * WORST_RMS and pos1 <= 2.0 * WORST_POS
    for k in range(4):
        assert err[k] <= 2.0 * WORST_C[k], (k, err)


if __name__ == "__main__":
    print("| seed | generic rms | generic pos | adapted rms | adapted pos | c | max abs(c - c_true) |")
    rows = [measure(s) for s in TABLE_SEEDS]
    for s, (rms0, pos0, rms1, pos1, c) in zip(TABLE_SEEDS, rows):
        print(f"| {s} | {rms0:.3f} | {pos0:.2f} | {rms1:.3f} | {pos1:.2f} | {np.round(c, 4).tolist()} | {np.abs(c - np.array(ss.C_TRUE)).max():.4f} |")
    errs = np.array([np.abs(r[4] - np.array(ss.C_TRUE)) for r in rows])
    print("worst: rms", max(r[2] for r in rows), "pos", max(r[3] for r in rows), "c", errs.max(axis=0))
    sys.exit(0)
