"""The vote-support restatement (tests/support_ref.py) against the oracle's own accumulator, and the support ABI without a GPU.

* mass equals the sum of the oracle's `mid_cells` inside the cube m +- r, total_mass the sum of all of them (frames small
  enough that no cell wraps), for radius 0 / 10 / large, an all-zero frame, a hand-built frame with a known box, and a head
  at the frame edge.  Midpoint guesses on each frame's densest cell start the mean shift on the votes, so the cube holds
  some but not all of a frame's votes (support_ref.partial);
* plausibility on `training.synthetic_truth` frames, the mean shift started at the true head centre: at DH_SUPPORT_RADIUS
  the pose lands within 20 mm, the support box lies inside the head mask's box and overlaps it by the measured IoU bound,
  and the same frames' unguided poses, which never leave their initial guess, have no support;
* the new symbols are exported and declared, dh_support is 40 bytes, and the argument checks answer DH_EINVAL.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from depthhead_amd import synth
from depthhead_amd.forest import Forest, NODE_DTYPE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import support_ref as sr  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "depthhead_hip.h")
W, H = 160, 120


@pytest.fixture(scope="module")
def forest():
    return synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)


@pytest.fixture(scope="module")
def tables(forest):
    return sr.LeafTables(forest)


def cells_u64(res):
    c = res.mid_cells.astype(np.int64)
    c[:, 3] = res.mid_cells[:, 3].view(np.uint32)
    return c


def check_against_oracle(res, rec, radius):
    c = cells_u64(res)
    m = sr.as_i32_vec(res.mid_point)
    inside = np.all(np.abs(c[:, :3] - m[None, :]) <= radius, axis=1) if len(c) else np.zeros(0, dtype=bool)
    assert rec["total_mass"] == int(c[:, 3].sum())
    assert rec["mass"] == int(c[inside, 3].sum())
    assert (rec["mass"] > 0) <= (rec["hits"] > 0) and rec["windows"] <= rec["hits"]
    if rec["hits"] == 0:
        assert (rec["x"], rec["y"], rec["width"], rec["height"], rec["windows"]) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("radius", [0, 10, 1 << 30])
def test_restatement_matches_the_oracle_accumulator(oracle, forest, tables, radius):
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(W, H)
    frames = synth.biwi_batch(8, W, H, first=40)
    total, recs = 0, []
    for i in range(8):
        g = sr.densest_cell(oracle, forest, model, frames[i], K)
        res, rec, votes = sr.support_ref(oracle, tables, model, frames[i], K, radius, g)
        recs.append(sr.as_record(rec, np.dtype([(k, "<u8") for k in sr.SUPPORT_FIELDS])))
        assert res.mid_cells[:, 3].view(np.uint32).max(initial=0) < (1 << 31)          # no cell wraps at this size
        check_against_oracle(res, rec, radius)
        total += rec["total_mass"]
        if radius == 1 << 30:                                                   # every vote supports
            assert rec["mass"] == rec["total_mass"]
            assert rec["hits"] == len(np.unique(votes[0] * 1_000_003 + votes[1]))
    assert total > 0
    if radius == 10:
        assert sr.partial(np.array(recs)) >= 3


def test_all_zero_frame_gives_all_zeros(oracle, forest, tables):
    model = synth.ModelParams(stepwidth=4)
    res, rec, _ = sr.support_ref(oracle, tables, model, np.zeros((H, W), np.uint16), synth.default_intrinsic(W, H), 10)
    assert all(v == 0 for v in rec.values())


def hand_forest():
    """One tree, one split that every non-zero window takes to leaf 0 (prob 1, two offsets 10 mm apart in x)."""
    nodes = np.zeros(1, dtype=NODE_DTYPE)
    nodes[0]["r1"] = (0, 0, 1, 1)
    nodes[0]["r2"] = (0, 0, 1, 1)
    nodes[0]["threshold"] = -1.0          # r1 mean - r2 mean = 0 > -1: child_one
    nodes[0]["child_zero"] = ~1
    nodes[0]["child_one"] = ~0
    offsets = np.array([[0, 0, 100], [10, 0, 100], [0, 0, 0]], dtype=np.float32)
    rots = np.array([[0, 0, 0], [0, 0, 0]], dtype=np.float64)
    return Forest(np.array([0], np.int32), nodes, np.array([1.0, 0.0]), np.array([0, 2, 3], np.uint32),
                  np.array([0, 1, 2], np.uint32), offsets, rots)


def test_hand_case_known_box(oracle):
    """A 48 x 40 block of constant depth in a 96 x 80 frame, 8 x 8 windows at stride 4: every gated window whose centre pixel
    sees the block casts two votes in front of the camera (the others' votes have z < 0); with the whole accumulator in range
    the box is exactly those windows' centres: x 24 .. 68, y 20 .. 56."""
    f = hand_forest()
    tab = sr.LeafTables(f)
    model = synth.ModelParams(stepwidth=4, subimage_width=8, subimage_height=8)
    img = np.zeros((80, 96), np.uint16)
    img[20:60, 24:72] = 900
    K = synth.default_intrinsic(96, 80)
    res, rec, votes = sr.support_ref(oracle, tab, model, img, K, 1 << 20)
    check_against_oracle(res, rec, 1 << 20)
    voting = np.flatnonzero(res.patch_flags == 3)
    nx, _ = model.patch_grid(96, 80)
    cx, cy = 4 + (voting % nx) * 4, 4 + (voting // nx) * 4
    front = img[cy, cx] > 0
    voting, cx, cy = voting[front], cx[front], cy[front]
    assert (cx.min(), cx.max(), cy.min(), cy.max()) == (24, 68, 20, 56)
    assert (rec["x"], rec["y"]) == (cx.min(), cy.min())
    assert (rec["width"], rec["height"]) == (cx.max() - cx.min() + 1, cy.max() - cy.min() + 1)
    assert rec["windows"] == rec["hits"] == len(voting) > 0
    assert rec["total_mass"] == rec["mass"] == 2 * 500 * len(voting)
    # Small radii around the mode the mean shift reaches from a guess on the votes (the corner window's first vote).  A
    # window's two votes are 10 cells apart in x and neighbouring windows' votes some 60 cells apart, so the cube takes one
    # vote at r = 0 and 9, both at r = 10 (the bound is inclusive), and four windows at r = 80.
    g = sr.densest_cell(oracle, f, model, img, K)
    for radius, mass, windows, side in ((0, 500, 1, 1), (9, 500, 1, 1), (10, 1000, 1, 1), (80, 4000, 4, 5)):
        res0, rec0, _ = sr.support_ref(oracle, tab, model, img, K, radius, g)
        check_against_oracle(res0, rec0, radius)
        assert (rec0["mass"], rec0["windows"], rec0["hits"], rec0["width"], rec0["height"]) == (mass, windows, windows, side, side), (radius, rec0)
        assert (rec0["x"], rec0["y"]) == (24, 20) and rec0["total_mass"] == 2 * 500 * len(voting)


def test_head_at_the_frame_edge(oracle, forest, tables):
    """A head moved left until its supporting windows reach the first window column (centre x = subimage_width / 2)."""
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(W, H)
    fr = synth.biwi_batch(1, W, H, first=44)[0]
    edge = np.zeros_like(fr)
    edge[:, : W - W // 3] = fr[:, W // 3:]
    g = sr.densest_cell(oracle, forest, model, edge, K)
    recs = []
    for radius in (10, 60):
        res, rec, _ = sr.support_ref(oracle, tables, model, edge, K, radius, g)
        check_against_oracle(res, rec, radius)
        assert 0 < rec["mass"] < rec["total_mass"] and rec["windows"] > 1, rec
        assert rec["x"] >= model.subimage_width // 2 and rec["x"] + rec["width"] - 1 <= W - model.subimage_width // 2
        recs.append(rec)
    assert recs[1]["x"] == model.subimage_width // 2 and recs[1]["windows"] > recs[0]["windows"]


def test_support_box_is_plausible_on_synthetic_heads(oracle, forest, tables):
    """Bounds measured on these 16 frames at DH_SUPPORT_RADIUS = 30: pose error at most 16.3 mm,
    support box wholly inside the mask's box, IoU with it at least 0.058 (mean 0.278), at least 5 windows, confidence at
    least 0.0209; no unguided pose has support."""
    from depthhead_amd import _lib, training
    model = synth.ModelParams(stepwidth=4)
    r = _lib.SUPPORT_RADIUS
    ious = []
    for i in range(16):
        depth, mask, K, pos3d, _ = training.synthetic_truth(320, 240, synth.FRAME_SEED_BASE + 1000 + i)
        res, rec, _ = sr.support_ref(oracle, tables, model, depth, K, r, pos3d)
        assert np.linalg.norm(res.mid_point - pos3d) < 20.0, i
        assert rec["windows"] >= 5 and rec["mass"] >= 0.02 * rec["total_mass"] > 0, (i, rec)
        ys, xs = np.nonzero(mask)
        mx0, my0, mx1, my1 = xs.min(), ys.min(), xs.max(), ys.max()
        bx0, by0, bx1, by1 = rec["x"], rec["y"], rec["x"] + rec["width"] - 1, rec["y"] + rec["height"] - 1
        assert mx0 <= bx0 and bx1 <= mx1 and my0 <= by0 and by1 <= my1, (i, rec, (mx0, my0, mx1, my1))
        area = lambda x0, y0, x1, y1: (x1 - x0 + 1) * (y1 - y0 + 1)   # noqa: E731
        ious.append(area(bx0, by0, bx1, by1) / area(mx0, my0, mx1, my1))   # (the box is inside: intersection = box)
        _, rec0, _ = sr.support_ref(oracle, tables, model, depth, K, r)   # no guess: the mean shift stays where it started
        assert rec0["mass"] == 0 and rec0["total_mass"] > 0, (i, rec0)
    assert min(ious) >= 0.05 and np.mean(ious) >= 0.25, ious


# ---------------------------------------------------------------------------------------------------- ABI without a GPU
SUPPORT_CALLS = ["dh_predict_batch_support", "dh_predict_batch_support_device", "dh_predict_batch_cameras_support",
                 "dh_predict_batch_cameras_support_device", "dh_tracker_step_support", "dh_tracker_step_support_device"]


def test_support_symbols_and_layout(hip_lib):
    from depthhead_amd import _lib
    src = open(HEADER).read()
    for name in SUPPORT_CALLS:
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS and f"int {name}(" in src
    assert _lib.SUPPORT_DTYPE.itemsize == 40 and _lib.SUPPORT_DTYPE.fields["mass"][1] == 24
    assert _lib.SUPPORT_DTYPE.alignment == _lib.POSE_DTYPE.alignment
    assert f"#define DH_SUPPORT_RADIUS {_lib.SUPPORT_RADIUS} " in src


def test_support_argument_checks_without_gpu(hip_lib):
    lib = hip_lib
    fr = np.zeros((1, 8, 8), np.uint16)
    out = np.zeros(1, dtype=np.uint8).repeat(40)
    sup = np.zeros(40, np.uint8)
    K = (C.c_float * 9)(*([1.0] * 9))
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    r = C.c_uint32
    # a negative radius (wrapped to uint32) is refused first, with its own message
    assert lib.dh_predict_batch_support(None, vp(fr), 1, 8, 8, K, None, None, None, r(0xFFFFFFFF), vp(out), vp(sup)) == -1
    assert b"radius" in lib.dh_last_error()
    assert lib.dh_predict_batch_support_device(None, vp(fr), 1, 8, 8, K, None, None, None, r(1 << 31), vp(out), vp(sup), None) == -1
    assert b"radius" in lib.dh_last_error()
    # NULL support / predictor / tables
    assert lib.dh_predict_batch_support(None, vp(fr), 1, 8, 8, K, None, None, None, r(10), vp(out), None) == -1
    assert b"NULL support" in lib.dh_last_error()
    assert lib.dh_predict_batch_support(None, vp(fr), 1, 8, 8, K, None, None, None, r(10), vp(out), vp(sup)) == -1
    assert lib.dh_predict_batch_cameras_support(None, vp(fr), 1, 8, 8, None, None, None, None, r(10), vp(out), vp(sup)) == -1
    assert lib.dh_predict_batch_cameras_support_device(None, vp(fr), 1, 8, 8, None, None, None, None, r(10), vp(out), vp(sup), None) == -1
    assert lib.dh_tracker_step_support(None, None, vp(fr), 8, 8, None, r(10), vp(out), vp(sup)) == -1
    assert lib.dh_tracker_step_support_device(None, None, vp(fr), 8, 8, None, r(0xFFFFFFFF), vp(out), vp(sup), None) == -1
    assert b"radius" in lib.dh_last_error()
