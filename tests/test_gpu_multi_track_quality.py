"""Quality of the multi-head tracker's identities: two synthetic heads in one 320 x 240 scene, the
second moving 2 pixels per step across 12 steps, the 6-tree test forest at stride 4 (section 14's quality setting).  In the
pinned scenes the heads pipeline finds a head near each true head at every step, and the id of the head nearest each true
head never changes.  The scenes and the bound were picked from a measured run of tools/multi_track_quality.py."""
import numpy as np
import pytest

from depthhead_amd import synth

pytestmark = pytest.mark.gpu

W, H = 320, 240
STEPS = 12
FOREST_ARGS = (6, 10, synth.FOREST_SEED_BASE + 9)
# The measured run (candidates first = 0 .. 23): in 9 scenes a detected head lay within 71.5 mm of both true heads at every step
# and the two were distinct; in the other 15 one true head was 217 - 920 mm from every detected head at some step (moved out of
# the frame or without a mode in the small forest's votes).  All 9 kept their two ids; the bound leaves a 25 % margin.
PINNED = [1, 2, 4, 7, 9, 15, 17, 18, 22]
BOUND = 90.0


def scenes(firsts, steps=STEPS, w=W, h=H):
    """(frames [steps, n, h, w], truths [steps, n, 2, 3] in mm): scene i holds stream frame firsts[i] and stream frame
    firsts[i] + 500 moved right (left for odd firsts[i]) by a third of the width plus 2 pixels per step."""
    from depthhead_amd import training
    n = len(firsts)
    frames = np.empty((steps, n, h, w), dtype=np.uint16)
    truths = np.empty((steps, n, 2, 3), dtype=np.float64)
    for i, f in enumerate(firsts):
        da, _, K, pa, _ = training.synthetic_truth(w, h, synth.FRAME_SEED_BASE + f)
        db, _, _, pb, _ = training.synthetic_truth(w, h, synth.FRAME_SEED_BASE + f + 500)
        fx = float(K[0, 0])
        for k in range(steps):
            s = (w // 3 + 2 * k) * (-1 if f % 2 else 1)
            moved = np.zeros_like(db)
            if s >= 0:
                moved[:, s:] = db[:, : w - s]
            else:
                moved[:, : w + s] = db[:, -s:]
            both = (da > 0) & (moved > 0)
            frames[k, i] = np.where(both, np.minimum(da, moved), np.maximum(da, moved))
            truths[k, i, 0] = pa
            truths[k, i, 1] = pb + np.array([s * float(pb[2]) / fx, 0.0, 0.0])
    return frames, truths


def evaluate(hp, tracking, cams, frames, truths, max_heads=4, radius=30):
    """Per scene: worst distance (mm) from a true head to its nearest detected head over the steps, whether the two nearest
    heads were always distinct, and the ids of the nearest heads per step."""
    n = frames.shape[1]
    worst = np.zeros(n)
    distinct = np.ones(n, dtype=bool)
    ids = np.zeros((frames.shape[0], n, 2), dtype=np.int64)
    with tracking.MultiHeadTracker(hp, cams, frames.shape[3], frames.shape[2], max_heads, radius) as tr:
        for k in range(frames.shape[0]):
            nh, heads, hid, _ = tr.step(frames[k], tracks=False)
            for i in range(n):
                m = int(nh[i])
                if m == 0:
                    worst[i] = np.inf
                    distinct[i] = False
                    continue
                mids = heads[i, :m]["pose"]["mid_point"].astype(np.float64)
                near = []
                for t in range(2):
                    d = np.linalg.norm(mids - truths[k, i, t], axis=1)
                    j = int(np.argmin(d))
                    worst[i] = max(worst[i], float(d[j]))
                    near.append(j)
                    ids[k, i, t] = int(hid[i, j])
                distinct[i] &= near[0] != near[1]
    held = [bool(distinct[i] and (ids[:, i] == ids[0, i]).all() and (ids[0, i] != 0).all()) for i in range(n)]
    return worst, distinct, ids, held


def test_identities_hold_on_moving_heads(hip_lib):
    from depthhead_amd import prediction, tracking
    forest = synth.fit_forest(*FOREST_ARGS, n_frames=12, subset=1500)
    frames, truths = scenes(PINNED)
    K = synth.default_intrinsic(W, H)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, \
            tracking.Cameras(np.repeat(K[None], len(PINNED), 0)) as cams:
        worst, distinct, ids, held = evaluate(hp, tracking, cams, frames, truths)
    for i, f in enumerate(PINNED):
        assert worst[i] <= BOUND, (f, worst[i])
        assert distinct[i], f
        assert held[i], (f, ids[:, i].tolist())
