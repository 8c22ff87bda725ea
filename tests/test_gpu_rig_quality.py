"""Quality of the rig tracker on two views of one scene.

Two cameras with parallel axes, R = I, t_A = 0, t_B = (b, 0, 0).  Camera A sees the two-head scene of section 15's quality test
(tests/test_gpu_multi_track_quality.py: two synthetic heads in 320 x 240, the second moving 2 pixels per step over 12 steps);
camera B sees the same frame moved left by an integer disparity of DISPARITY pixels, and b = DISPARITY * z / f_x with z the mean
true depth of the two heads.  The scene is heads over an empty background, so a shift IS the second view up to the heads' own
depth range: a head at depth z' has the disparity b f_x / z', which differs from DISPARITY by (z - z') / z' of it; that
approximation is part of the setting.  The ground truth in the world frame is camera A's truth.  The rig tracker runs with
max_heads 2 (the scenes hold two heads), r = 30, the default fuse gate, gate and misses; camera B is marked absent at steps
ABSENT_B and camera A at steps ABSENT_A.

The scenes were chosen on the CPU, before any GPU run, by tools/rig_track_quality.py: the CPU restatement (tests/heads_ref.py
on the C oracle's taps, then tests/rig_track_ref.py) finds both true heads in both views at every step (two heads per view, the
nearest head to each truth distinct and within FOUND_MM).  On the kept scenes the GPU must give: at every step exactly two
persons, each with two views (one view where a camera is absent); the id of the person nearest each true head never changes
over the 12 steps; every person's cell within BOUND of the true world position."""
import os
import sys

import numpy as np
import pytest

from depthhead_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_multi_track_quality as q15  # noqa: E402

W, H, STEPS, FOREST_ARGS = q15.W, q15.H, q15.STEPS, q15.FOREST_ARGS
DISPARITY = 20                 # pixels
MAX_HEADS, RADIUS = 2, 30
ABSENT_B = (4, 5)              # steps at which camera B is absent
ABSENT_A = (8,)                # steps at which camera A is absent
FOUND_MM = 100.0               # "found": a detected head within the fuse gate's 100 mm of the truth (the header's reason for the gate)
CANDIDATES = list(range(0, 424))
# The measured CPU run (tools/rig_track_quality.py --cpu --first 0 --count 424, no GPU involved).  The first 72 candidates gave
# one scene, fewer than the four the test needs, so the list was widened to 424 with the criterion as it stood: 8 scenes
# qualify.  In the other 416 the two heaviest heads of some view at some step are not the two true heads: the 6-tree forest's
# votes also pile up behind the heads, and such a spurious head outweighs the farther true one (worst distances 98 - 1007 mm),
# or a head leaves the frame.  On the 8 kept scenes the restatement gives two persons with the expected views at every step,
# both ids held, and a worst Chebyshev distance of a person's cell from the true world position of 39.5 - 53.7 mm per scene.
KEPT = [26, 114, 122, 165, 221, 271, 341, 404]
WORST_MM = 53.7                # worst Chebyshev distance of a person's cell from the true world position over the kept scenes
BOUND = 67.2                   # WORST_MM with the 25 % margin sections 14 and 15 give theirs


def two_views(firsts):
    """(frames [steps, 2 n, H, W] with cameras 2 i (A) and 2 i + 1 (B) of scene i, world truths [steps, n, 2, 3], t [2 n, 3])"""
    fa, truths = q15.scenes(firsts)
    n = len(firsts)
    frames = np.zeros((STEPS, 2 * n, H, W), dtype=np.uint16)
    frames[:, 0::2] = fa
    frames[:, 1::2, :, : W - DISPARITY] = fa[:, :, :, DISPARITY:]
    fx = float(synth.default_intrinsic(W, H)[0, 0])
    t = np.zeros((2 * n, 3), dtype=np.float32)
    for i in range(n):
        t[2 * i + 1, 0] = np.float32(DISPARITY * float(truths[:, i, :, 2].mean()) / fx)
    return frames, truths, t


def presence(n):
    p = np.ones((STEPS, 2 * n), dtype=np.uint8)
    for k in ABSENT_B:
        p[k, 1::2] = 0
    for k in ABSENT_A:
        p[k, 0::2] = 0
    return p


def judge(n_persons, persons, present, truths):
    """One scene's steps (n_persons [steps], persons [steps, 16], present [steps, 2], truths [steps, 2, 3]) ->
    dict(two_persons, views_ok, ids [steps, 2], ids_held, worst_mm (Chebyshev, cell against truth), fused_err, per-person)"""
    out = dict(two_persons=True, views_ok=True, ids=np.zeros((STEPS, 2), np.int64), worst_mm=0.0)
    for k in range(STEPS):
        m = int(n_persons[k])
        want_views = int(present[k].sum())
        out["two_persons"] &= m == 2
        if m == 0:
            out["worst_mm"] = np.inf
            continue
        ps = persons[k][:m]
        out["views_ok"] &= bool((ps["n_views"] == want_views).all())
        cells = ps["cell"].astype(np.float64)
        near = []
        for h in range(2):
            d = np.abs(cells - truths[k, h]).max(axis=1)
            j = int(np.argmin(d))
            near.append(j)
            out["ids"][k, h] = int(ps["id"][j])
            out["worst_mm"] = max(out["worst_mm"], float(d[j]))
        out["two_persons"] &= near[0] != near[1]
    ids = out["ids"]
    out["ids_held"] = bool((ids == ids[0]).all() and (ids[0] != 0).all() and ids[0, 0] != ids[0, 1])
    return out


def rig_of(tracking, cams, t, n):
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2 * n, 1))
    return tracking.Rig(cams, eye, t, list(range(0, 2 * n + 1, 2)))


@pytest.mark.gpu
def test_fused_identities_hold_on_two_views(hip_lib):
    from depthhead_amd import prediction, tracking
    assert len(KEPT) >= 4, "the issue's condition: at least 4 scenes qualify"
    forest = synth.fit_forest(*FOREST_ARGS, n_frames=12, subset=1500)
    frames, truths, t = two_views(KEPT)
    present = presence(len(KEPT))
    K = synth.default_intrinsic(W, H)
    n = len(KEPT)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, \
            tracking.Cameras(np.repeat(K[None], 2 * n, 0)) as cams, rig_of(tracking, cams, t, n) as rig, \
            tracking.RigTracker(hp, rig, W, H, MAX_HEADS, RADIUS) as tr:
        outs = [tr.step(frames[k], present[k]) for k in range(STEPS)]
    for i, f in enumerate(KEPT):
        res = judge([o[3][i] for o in outs], [o[4][i] for o in outs], present[:, 2 * i:2 * i + 2], truths[:, i])
        print("scene", f, "worst_mm", res["worst_mm"], "ids", res["ids"].tolist())
        assert res["two_persons"], (f, [int(o[3][i]) for o in outs])
        assert res["views_ok"], (f, [o[4][i]["n_views"][:2].tolist() for o in outs])
        assert res["ids_held"], (f, res["ids"].tolist())
        assert res["worst_mm"] <= BOUND, (f, res["worst_mm"], BOUND)
