"""Adversarial input families shared by tests/test_edge_pyref.py (CPU: the two restatements against each other, the oracle
under the sanitizers) and tests/test_gpu_edge_families.py (the HIP path against both restatements).

Each family is a small seeded function returning a `Family`: forest, model, frames (uint16 [n, h, w], at most about
160 x 128 so that oracle/pyref.py stays fast), the intrinsic matrix and per-frame guess overrides.  The generator asserts on
its inputs that the edge is there; `reach(results)` asserts on the restatement's results (oracle/pyref.py, one dict per
frame) that the edge is actually reached, so that a family cannot silently turn benign.

FAMILIES drive the 3-D path (predict_parameter_generic, prediction.rs:421-753); AUX_FAMILIES drive the sibling consumers
(predict_mask :850-905, build_hough_image :760-845, predict_parameter_from2dhough :343-367).  Several families restate
inputs that the older GPU tests build inline (test_gpu_parity.py, test_gpu_round2.py, test_gpu_round3.py)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable

import numpy as np

from depthhead_amd import synth
from depthhead_amd.forest import NODE_DTYPE, Forest
from oracle import pyref

F64 = np.float64


@dataclass
class Family:
    forest: Forest
    model: synth.ModelParams
    frames: np.ndarray                 # uint16 [n, h, w]
    K: np.ndarray                      # float32 [3, 3]
    midp: np.ndarray | None = None     # float32 [n, 3]: midp_guess of every frame
    rot: np.ndarray | None = None      # float64 [n, 3]: rot_guess of every frame
    reach: Callable[[list], None] = field(default=lambda results: None)

    def guesses(self, i):
        return (None if self.midp is None else self.midp[i]), (None if self.rot is None else self.rot[i])


def _forest(roots, nodes, prob, n_votes, offsets, rotations) -> Forest:
    begin = np.concatenate([[0], np.cumsum(n_votes)]).astype(np.uint32)
    return Forest(np.asarray(roots, dtype=np.int32), nodes, np.asarray(prob, dtype=np.float64), begin, begin.copy(), offsets, rotations)


def _frames(n, w, h, first):
    return synth.biwi_batch(n, w, h, first=first)


def _flat_and_saturated(frames):
    """Frame 1 flat (every box sum of the foreground equal: differences of exactly 0), frame 2 saturated (largest sums)."""
    frames = frames.copy()
    frames[1] = (frames[1] > 0) * 800
    frames[2] = np.where(frames[2] > 0, 65535, 0)
    return frames.astype(np.uint16)


def walk_stats(forest, model, img) -> dict:
    """Re-walk every foreground window the way pyref.walk does and count the node visits at each kind of threshold:
    `equal` -- avg(r1) - avg(r2) == threshold exactly (the split test `>` is false on it), `nan`, `inf`, and visits of a
    rectangle of zero area (average_value_in_rect returns 0.0 there, types.rs:335-338)."""
    img = np.asarray(img, dtype=np.uint16)
    h, w = img.shape
    st = dict(equal=0, nan=0, inf=0, empty=0, windows=0, background=0)
    for _, _, ox, oy in pyref._windows(model, w, h):
        if not pyref.average_value_in_rect(img, ox, oy, (0, 0, model.subimage_width, model.subimage_height)) > 0.0:
            st["background"] += 1
            continue
        st["windows"] += 1
        for t in range(forest.n_trees):
            cur = int(forest.roots[t])
            while cur >= 0:
                nd = forest.nodes[cur]
                thr = F64(nd["threshold"])
                for r in (nd["r1"], nd["r2"]):
                    st["empty"] += int((int(r[2]) - int(r[0])) * (int(r[3]) - int(r[1])) == 0)
                d = F64(pyref.average_value_in_rect(img, ox, oy, nd["r1"]) - pyref.average_value_in_rect(img, ox, oy, nd["r2"]))
                st["equal"] += int(d == thr)
                st["nan"] += int(np.isnan(thr))
                st["inf"] += int(np.isinf(thr))
                cur = int(nd["child_one"]) if d > thr else int(nd["child_zero"])
    return st


def _hits(results, leaves) -> int:
    """Number of (voting window, tree) pairs that ended in one of `leaves`."""
    n = 0
    for r in results:
        voting = r["patch_flags"] == 3
        n += int(np.isin(r["leaf_idx"][voting], list(leaves)).sum())
    return n


# ================================================================== 3-D path families
def hand_forest() -> Family:
    """test_gpu_parity._hand_forest: a single-leaf tree, zero-area rectangles, a one-vote leaf (covariance 0 / 0 = NaN: it
    never votes, meancov_estimation.rs:376), rotations that wrap at +-180 degrees, votes behind the camera (np.z < 0)."""
    nodes = np.zeros(3, dtype=NODE_DTYPE)
    nodes[0] = ((10, 10, 34, 34), (40, 40, 64, 64), 0.0, 1, ~0)
    nodes[1] = ((0, 0, 0, 0), (5, 5, 5, 30), -1.0, ~1, 2)
    nodes[2] = ((0, 0, 80, 80), (0, 0, 1, 1), 100.0, ~2, ~3)
    offsets = np.array([[10, 5, -20], [12, 6, -22], [9, 4, -19], [0, 0, 0],
                        [-30, 10, 15], [-31, 11, 16], [-29, 9, 14], [-30.5, 10.5, 15.5],
                        [1e6, 0, 0], [-1e6, 0, 0],
                        [0.5, 0.5, 2000.0], [0.25, 0.75, 1999.0], [0.1, 0.2, 2001.0]], dtype=np.float32)
    rotations = np.array([[181.0, -185.0, 10], [178.0, -178.0, 11], [179.9, -179.9, 9], [5, 5, 5],
                          [20, -30, 40], [21, -31, 41], [19, -29, 39], [20.5, -30.5, 40.5],
                          [0, 0, 0], [90, 90, 90],
                          [-2.9, 2.9, 0.0], [-3.1, 3.1, -0.0], [-1.0, 1.0, 0.5]], dtype=np.float64)
    forest = _forest([0, ~4], nodes, [0.9, 0.5, 1.0, 0.8, 1.0], [3, 1, 4, 2, 3], offsets, rotations)
    w, h = 160, 128
    frames = _frames(2, w, h, 5)

    def reach(results):
        cells = np.concatenate([r["rot_cells"] for r in results])
        assert ((cells[:, :3] == 0) | (cells[:, :3] == 119)).any()          # a rotation bin wrapped
        assert _hits(results, [0]) > 0 and _hits(results, [4]) > 0
    return Family(forest, synth.ModelParams(stepwidth=6, meanshift_iterations=7), frames, synth.default_intrinsic(w, h), reach=reach)


def integer_thresholds() -> Family:
    """test_gpu_parity.test_integer_threshold_edge_cases: uniform 24 x 24 rectangles, thresholds exactly on a reachable
    difference k / 576 and one ulp either side of it, 0, +-65535, +-1e9, +-inf; flat and saturated frames."""
    forest = synth.synth_forest(6, 9, synth.FOREST_SEED_BASE + 151)
    c = 24.0 * 24.0
    thr = forest.nodes["threshold"]
    exact = np.round(thr * c) / c
    sel = np.arange(thr.size) % 4
    thr[sel == 0] = exact[sel == 0]
    thr[sel == 1] = np.nextafter(exact[sel == 1], np.inf)
    thr[sel == 2] = np.nextafter(exact[sel == 2], -np.inf)
    thr[sel == 3] = np.where(np.arange(thr.size)[sel == 3] % 8 == 3, 0.0, thr[sel == 3])
    thr[5] = 1e9; thr[6] = -1e9; thr[7] = 65535.0; thr[8] = -65535.0; thr[9] = np.inf; thr[10] = -np.inf
    w, h = 160, 128
    frames = _flat_and_saturated(_frames(3, w, h, 33))
    model = synth.ModelParams(stepwidth=4)

    def reach(results):
        st = [walk_stats(forest, model, f) for f in frames]
        assert sum(s["equal"] for s in st) >= 50, st                 # d == threshold: the split goes to child_zero
        assert sum(s["inf"] for s in st) > 0
    return Family(forest, model, frames, synth.default_intrinsic(w, h), reach=reach)


def nonfinite_thresholds() -> Family:
    """Thresholds NaN (`d > NaN` is false: child_zero), +-inf, +-DBL_MAX, the smallest subnormals, -0.0 on frames where d = 0."""
    forest = synth.synth_forest(6, 9, synth.FOREST_SEED_BASE + 153)
    thr = forest.nodes["threshold"]
    kinds = np.array([np.nan, np.inf, -np.inf, np.finfo(np.float64).max, -np.finfo(np.float64).max, 5e-324, -5e-324, -0.0, 0.0])
    sel = np.arange(thr.size) % 3 == 0
    thr[sel] = kinds[np.arange(int(sel.sum())) % kinds.size]
    thr[forest.roots[forest.roots >= 0]] = np.nan                    # every root: NaN
    w, h = 160, 128
    frames = _flat_and_saturated(_frames(3, w, h, 41))
    model = synth.ModelParams(stepwidth=4)

    def reach(results):
        st = [walk_stats(forest, model, f) for f in frames]
        assert sum(s["nan"] for s in st) > 0 and sum(s["inf"] for s in st) > 0, st
    return Family(forest, model, frames, synth.default_intrinsic(w, h), reach=reach)


def blank_frames() -> Family:
    """test_gpu_parity.test_edge_frames: an all-background frame, a single non-zero pixel, a saturated frame."""
    forest = synth.synth_forest(4, 8, synth.FOREST_SEED_BASE + 5)
    w, h = 160, 120
    frames = np.zeros((3, h, w), dtype=np.uint16)
    frames[1, 60, 80] = 1
    frames[2] = 65535

    def reach(results):
        assert not results[0]["patch_flags"].any()                   # every window background
        assert (results[1]["patch_flags"] > 0).sum() > 0 and (results[1]["patch_flags"] == 0).sum() > 0
        assert (results[2]["patch_flags"] > 0).all()
    return Family(forest, synth.ModelParams(stepwidth=4), frames, synth.default_intrinsic(w, h), reach=reach)


def no_window_frame() -> Family:
    """w == h == patch side: the window loops run zero times (prediction.rs:535-548)."""
    forest = synth.synth_forest(4, 8, synth.FOREST_SEED_BASE + 5)
    frames = synth.biwi_batch(1, 160, 120)[:, :80, :80].copy()

    def reach(results):
        assert results[0]["leaf_idx"].shape[0] == 0
    return Family(forest, synth.ModelParams(stepwidth=4), frames, synth.default_intrinsic(80, 80), reach=reach)


def one_row_of_windows() -> Family:
    """An 83 x 81 frame at stepwidth 1: exactly one row of three window positions."""
    forest = synth.synth_forest(4, 8, synth.FOREST_SEED_BASE + 5)
    base = synth.biwi_like(640, 480, synth.FRAME_SEED_BASE + 3)
    ys, xs = np.nonzero(base)
    cy, cx = int(ys.mean()), int(xs.mean())
    frames = base[None, cy - 40:cy + 41, cx - 41:cx + 42].copy()

    def reach(results):
        assert results[0]["leaf_idx"].shape[0] == 3 and (results[0]["patch_flags"] > 0).all()
    return Family(forest, synth.ModelParams(stepwidth=1), frames, synth.default_intrinsic(83, 81), reach=reach)


def guess_overrides() -> Family:
    """The Option<> guesses of predict_parameter_generic (prediction.rs:437-460) at the limits of the casts: +-1e20, +-2^31,
    +-inf and NaN positions (`as i32` saturates, NaN -> 0); rotations of 1e300, +-inf, NaN and ones that land on +-2^31."""
    forest = synth.synth_forest(6, 9, synth.FOREST_SEED_BASE + 4)
    w, h = 160, 128
    frames = _frames(4, w, h, 20)
    big = 2.0 ** 31
    midp = np.array([[1e20, -1e20, np.nan], [big, -big, np.inf], [-np.inf, big - 128, -(big + 256)], [12.7, -30.2, 905.9]], dtype=np.float32)
    # guess_rot = ((g * 180 / 3.14159 + 180) * 120 / 360) as i32: 3.14159 * (3 * 2^31 - 180) / 180 reaches i32::MAX
    g31 = (3.0 * big - 180.0) * 3.14159 / 180.0
    rot = np.array([[1e300, -7.0, np.nan], [np.inf, -np.inf, 0.0], [g31, -g31, 2 * g31], [0.3, -0.2, 1.1]], dtype=np.float64)

    def reach(results):
        gm = np.stack([r["guess_mid"] for r in results])
        gr = np.stack([r["guess_rot"] for r in results])
        assert (gm == 2147483647).any() and (gm == -2147483648).any() and (gm == 0).any()
        assert (gr == 2147483647).any() and (gr == -2147483648).any()
    return Family(forest, synth.ModelParams(stepwidth=5), frames, synth.default_intrinsic(w, h), midp, rot, reach=reach)


def odd_patch_dense_intrinsic() -> Family:
    """test_gpu_parity.test_non_square_odd_patch_and_dense_intrinsic: a 61 x 47 patch (left / right halves differ,
    prediction.rs:535-538) and the dense intrinsic matrix of the reference's own test (types.rs:478)."""
    forest = synth.synth_forest(5, 9, synth.FOREST_SEED_BASE + 6, patch=(61, 47))
    model = synth.ModelParams(stepwidth=3, subimage_width=61, subimage_height=47, gaussian_sigma=3.5, meanshift_iterations=5)
    K = np.array([[22.0, 11.4, 12.11], [2.1, 4.1, 2.11], [1.3, 3.1, 19.0]], dtype=np.float32)
    frames = _frames(2, 150, 120, 7)

    def reach(results):
        assert sum(len(r["mid_cells"]) for r in results) > 0
    return Family(forest, model, frames, K, reach=reach)


def window_means_at_the_gate() -> Family:
    """test_gpu_round2.test_window_means_at_the_gate: leaf probabilities chosen so that window means sit exactly on, and one
    ulp beside, 0.7 (prediction.rs:582-584: tree-order f64 sum, `> 0.7`)."""
    rs = np.random.RandomState(5)
    forest = synth.synth_forest(10, 6, synth.FOREST_SEED_BASE + 22)
    prob = forest.leaf_prob
    voting = prob > 0
    choices = np.array([0.7, np.nextafter(0.7, 1.0), np.nextafter(0.7, 0.0), 0.75, 0.65, 1.0, 0.7000001, 0.6999999])
    prob[voting] = choices[rs.randint(0, choices.size, int(voting.sum()))]
    w, h = 160, 128
    frames = _frames(3, w, h, 60)

    def reach(results):
        means = []
        for r in results:
            for row in r["leaf_idx"][r["patch_flags"] > 0]:
                s = F64(0.0)
                for L in row:
                    s = F64(s + F64(prob[L]))
                means.append(F64(s / F64(len(row))))
        means = np.array(means)
        assert (means > 0.7).any() and (means <= 0.7).any()
        near = np.abs(means - 0.7) <= 4 * np.spacing(0.7)
        assert near.sum() > 0, "no window mean within 4 ulp of the gate"
    return Family(forest, synth.ModelParams(stepwidth=3), frames, synth.default_intrinsic(w, h), reach=reach)


def probabilities_outside_the_unit_interval() -> Family:
    """test_gpu_round2.test_leaf_probabilities_outside_the_unit_interval, extended: leaf 'probabilities' of 1.9 x, 1e300
    (1000 * p saturates `as usize`, prediction.rs:590), +inf and NaN (the window mean is NaN: `> 0.7` is false)."""
    forest = synth.synth_forest(6, 6, synth.FOREST_SEED_BASE + 23)
    prob = forest.leaf_prob
    pos = np.flatnonzero(prob > 0.5)
    prob[prob > 0] *= 1.9
    special = {1e300: pos[0::7], np.inf: pos[3::7], np.nan: pos[5::11]}
    for v, idx in special.items():
        prob[idx] = v
    assert np.nanmax(prob[np.isfinite(prob)]) > 1.0
    w, h = 160, 128
    frames = _frames(3, w, h, 64)

    def reach(results):
        assert _hits(results, special[1e300]) > 0 and _hits(results, special[np.inf]) > 0
        nan_windows = sum(int(np.isin(r["leaf_idx"][r["patch_flags"] > 0], special[np.nan]).any(axis=1).sum()) for r in results)
        assert nan_windows > 0
    return Family(forest, synth.ModelParams(stepwidth=4), frames, synth.default_intrinsic(w, h), reach=reach)


def nonfinite_offset_votes() -> Family:
    """test_gpu_round2.test_pinhole_projection_falls_back_for_huge_and_non_finite_votes: offsets of 3e35, -inf, +inf and NaN
    (0 * inf = NaN propagates through space_to_img_coord, types.rs:424-428)."""
    rs = np.random.RandomState(11)
    forest = synth.fit_forest(6, 8, synth.FOREST_SEED_BASE + 41, n_frames=10, subset=1200)
    voting = np.flatnonzero(forest.leaf_prob > 0)
    touched = []
    for L in voting[rs.rand(voting.size) < 0.3]:
        ob, oe = int(forest.off_begin[L]), int(forest.off_begin[L + 1])
        kind = rs.randint(0, 4)
        k = ob + rs.randint(0, oe - ob)
        if kind == 0:
            forest.offsets[k] = [3.0e35, -2.0e33, 1.0e31]
        elif kind == 1:
            forest.offsets[k, 2] = -np.inf
        elif kind == 2:
            forest.offsets[k, 0] = np.inf
        else:
            forest.offsets[k] = [np.nan, 0.0, -50.0]
        touched.append(L)
    w, h = 160, 128
    frames = _frames(3, w, h, 70)

    def reach(results):
        assert _hits(results, touched) > 0
    return Family(forest, synth.ModelParams(stepwidth=4), frames, synth.default_intrinsic(w, h), reach=reach)


def mixed_rectangles_on_reachable_differences() -> Family:
    """test_gpu_round2.test_mixed_rectangles_with_thresholds_on_reachable_differences: rectangles of different sizes
    (c1 != c2), thresholds on k / (c1 c2) and one ulp beside it, 0, +-65535, +-inf, and rectangles of zero area."""
    forest = synth.synth_forest(7, 9, synth.FOREST_SEED_BASE + 152, rect_scale=0.08, rect_scale_max=0.7)
    nd = forest.nodes
    c1 = (nd["r1"][:, 2].astype(np.int64) - nd["r1"][:, 0]) * (nd["r1"][:, 3].astype(np.int64) - nd["r1"][:, 1])
    c2 = (nd["r2"][:, 2].astype(np.int64) - nd["r2"][:, 0]) * (nd["r2"][:, 3].astype(np.int64) - nd["r2"][:, 1])
    assert (c1 != c2).mean() > 0.5
    cc = (np.maximum(c1, 1) * np.maximum(c2, 1)).astype(np.float64)
    thr = nd["threshold"]
    exact = np.round(thr * cc) / cc
    sel = np.arange(thr.size) % 5
    thr[sel == 0] = exact[sel == 0]
    thr[sel == 1] = np.nextafter(exact[sel == 1], np.inf)
    thr[sel == 2] = np.nextafter(exact[sel == 2], -np.inf)
    thr[sel == 3] = 0.0
    thr[11] = 65535.0; thr[12] = -65535.0; thr[13] = np.inf; thr[14] = -np.inf; thr[15] = np.nextafter(65535.0, 0.0)
    nd["r1"][20, 2] = nd["r1"][20, 0]
    nd["r2"][21, 3] = nd["r2"][21, 1]
    nd["r1"][22, 2] = nd["r1"][22, 0]; nd["r2"][22, 2] = nd["r2"][22, 0]
    for i in range(forest.n_trees):                                   # the roots too: every window visits a zero-area rectangle
        r = forest.roots[i]
        if r >= 0 and i % 2 == 0:
            nd["r2"][r, 3] = nd["r2"][r, 1]
    w, h = 160, 128
    frames = _flat_and_saturated(_frames(3, w, h, 37))
    model = synth.ModelParams(stepwidth=4)

    def reach(results):
        st = [walk_stats(forest, model, f) for f in frames]
        assert sum(s["equal"] for s in st) > 0 and sum(s["empty"] for s in st) > 0, st
    return Family(forest, model, frames, synth.default_intrinsic(w, h), reach=reach)


def hundreds_of_equal_rotations() -> Family:
    """test_gpu_round3.test_leaves_with_hundreds_of_equal_rotations: leaves holding 700 / 256 / 255 / 300 + 300 / 1 / 511
    rotations, most of them equal (rotation bins with more than 255 votes of one leaf)."""
    nodes = np.zeros(3, dtype=NODE_DTYPE)
    nodes[0] = ((4, 4, 28, 28), (40, 40, 64, 64), 0.0, ~0, ~1)
    nodes[1] = ((10, 30, 34, 54), (44, 6, 68, 30), 10.0, ~2, ~3)
    nodes[2] = ((0, 0, 24, 24), (56, 56, 80, 80), -5.0, ~4, ~5)
    n = [700, 256, 255, 600, 1, 511]
    begin = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
    rs = np.random.RandomState(11)
    centre = rs.uniform(-20, 20, (6, 3))
    rotations = np.repeat(centre, n, axis=0)
    rotations[int(begin[3]) + 300:int(begin[4])] += 3.0
    rotations[int(begin[0]):int(begin[0]) + 40] += rs.uniform(-6, 6, (40, 3))
    offsets = (np.repeat(rs.uniform(-30, 30, (6, 3)), n, axis=0) + rs.uniform(-1, 1, (int(begin[-1]), 3))).astype(np.float32)
    forest = _forest([0, 1, 2], nodes, [1.0, 0.9, 0.95, 1.0, 0.8, 1.0], n, offsets, rotations)
    base = synth.biwi_like(640, 480, 777)
    ys, xs = np.nonzero(base)
    cy, cx = int(ys.mean()), int(xs.mean())
    frames = np.stack([base[cy - 60:cy + 60, cx - 70:cx + 70], base[cy - 40:cy + 80, cx - 90:cx + 50]]).copy()

    def reach(results):
        assert max(int(r["rot_cells"][:, 3].astype(np.uint32).max(initial=0)) for r in results) > 255 * 1   # 700 equal votes x valtoadd
        assert _hits(results, [0]) > 0 and _hits(results, [3]) > 0
    return Family(forest, synth.ModelParams(stepwidth=8), frames, synth.default_intrinsic(140, 120), reach=reach)


def vote_cells_at_grid_borders() -> Family:
    """test_gpu_round2.test_vote_cells_at_grid_borders at 200 x 160: a flat frame at z = fx puts every vote ON, or 1e-6 ..
    1e-2 pixels beside, a border of the 20 x 20 guess grid; a one-leaf forest that every window hits."""
    w, h = 200, 160
    K = synth.default_intrinsic(w, h)
    fx = float(K[0, 0])
    assert fx == int(fx)
    frames = np.full((2, h, w), int(fx), dtype=np.uint16)
    frames[1, :, : w // 2] = 0
    eps = [0.0, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 3e-4, -3e-4, 1e-3, -1e-3, 1e-2]
    cw, ch = w / 20.0, h / 20.0
    offs = np.array([[(40 % cw) + 4 * (j % 3) + e, (40 % ch) + 4 * (j % 2) - e, 0.0] for j, e in enumerate(eps)], dtype=np.float32)
    rots = np.tile(np.array([[0.1, -0.2, 0.3]]), (2, 1))
    forest = Forest(np.array([~0], dtype=np.int32), np.zeros(0, dtype=NODE_DTYPE), np.array([1.0]),
                    np.array([0, len(offs)], dtype=np.uint32), np.array([0, len(rots)], dtype=np.uint32), offs, rots)

    def reach(results):
        assert results[0]["pos_grid"].astype(np.int64).sum() > 0 and (results[1]["patch_flags"] == 0).any()
    return Family(forest, synth.ModelParams(stepwidth=4), frames, K, reach=reach)


# ---- k_vote's approximate cell quotient, emulated in numpy float32 (depthhead_amd/csrc/k_vote.hip, vote_positions)
def window_points(K, model, frame):
    """img_to_space (types.rs:432-445) of the centre of every foreground window of `frame` (the ones that vote), in the
    reference's window order: float32 [n, 3]."""
    h, w = frame.shape
    box = (0, 0, model.subimage_width, model.subimage_height)
    xy = np.array([(x, y) for x, y, ox, oy in pyref._windows(model, w, h) if pyref.average_value_in_rect(frame, ox, oy, box) > 0.0],
                  dtype=np.int64).reshape(-1, 2)
    x, y, z = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32), frame[xy[:, 1], xy[:, 0]].astype(np.float32)
    inv = pyref.mat3_inv(np.asarray(K, dtype=np.float32), np.float32)
    r = []
    for j in range(3):                                                  # meancov_estimation.rs:201-216, operation by operation
        t = x * inv[j][0]
        t = t + y * inv[j][1]
        r.append(t + np.float32(1.0) * inv[j][2])
    with np.errstate(all="ignore"):
        c = z / r[2]
        return np.stack([r[0] * c, r[1] * c, r[2] * c], axis=-1)


def _fma_f32(a, b, c):
    """fmaf(a, b, c) with one rounding: a * b of two floats is exact in float64; the float64 sum is rounded to odd (TwoSum
    gives its error), which then rounds to the float32 of the exact a * b + c."""
    p = a.astype(F64) * b.astype(F64)
    s = p + F64(c)
    bb = s - p
    with np.errstate(invalid="ignore"):
        err = (p - (s - bb)) + (F64(c) - bb)
    inexact = np.isfinite(s) & (err != 0) & (s.view(np.int64) & 1 == 0)
    s = np.where(inexact, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def vote_cells(K, w, h, p3, offs):
    """Guess-grid cells of every (window, offset) position vote: (votes [n, m] bool, the reference's cells (prediction.rs:647-672),
    [the cells vote_positions' PINNED fast path gives with v_rcp_f32 returning RN(1 / nz) - 1 ulp, RN, RN + 1 ulp]).  The fast
    path is fma(nx * rcp(nz), kxs, cxs) with kxs .. cys rounded once in f32 from 20 / w; quotients within 1e-4 of an integer
    fall back to the reference's expression, which is what the fast cells hold there."""
    K = np.asarray(K, dtype=np.float32)
    with np.errstate(all="ignore"):
        n = p3[:, None, :] - offs[None, :, :]
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]

        def ref_axis(row, lim):
            r = nx * K[row, 0]
            r = r + ny * K[row, 1]
            r = r + nz * K[row, 2]
            r2 = nx * K[2, 0]
            r2 = r2 + ny * K[2, 1]
            r2 = r2 + nz * K[2, 2]
            q = r / r2
            q = np.where(q > 0, q, np.float32(0.0))
            q = np.where(q < np.float32(lim - 1), q, np.float32(lim - 1))
            return q.astype(np.int64) * 20 // lim
        ref = ref_axis(1, h) * 20 + ref_axis(0, w)
        sx, sy = np.float32(20.0) / np.float32(w), np.float32(20.0) / np.float32(h)
        kxs, cxs, kys, cys = K[0, 0] * sx, K[0, 2] * sx, K[1, 1] * sy, K[1, 2] * sy
        rn = np.float32(1.0) / nz
        fast = []
        for rc in (np.nextafter(rn, np.float32(-np.inf)), rn, np.nextafter(rn, np.float32(np.inf))):
            ux, uy = _fma_f32(nx * rc, kxs, cxs), _fma_f32(ny * rc, kys, cys)
            near = ~(np.abs(ux - np.rint(ux)) > np.float32(1e-4)) | ~(np.abs(uy - np.rint(uy)) > np.float32(1e-4))
            cell = (np.minimum(np.maximum(uy, 0), 19.5).astype(np.int64) * 20 + np.minimum(np.maximum(ux, 0), 19.5).astype(np.int64))
            fast.append(np.where(near, ref, cell))
    return nz >= 0, ref, fast


def _one_leaf_forest(offs):
    rots = np.tile(np.array([[0.1, -0.2, 0.3]]), (2, 1))
    return Forest(np.array([~0], dtype=np.int32), np.zeros(0, dtype=NODE_DTYPE), np.array([1.0]),
                  np.array([0, len(offs)], dtype=np.uint32), np.array([0, len(rots)], dtype=np.uint32), offs, rots)


def _pos_grid(votes, cells, valtoadd):
    return np.bincount(cells[votes], minlength=400).astype(np.uint32) * np.uint32(valtoadd)


def _one_leaf_offsets_ok(offs):
    assert len(offs) >= 2 and np.isfinite(offs).all()
    assert pyref.trace_of_cov(offs, np.float32) <= pyref.MAX_VARIANCE_OFFSET       # prediction.rs:641: the leaf votes


def principal_point_beside_the_frame() -> Family:
    """vote_cells_at_grid_borders with the principal point two frame widths left of and 2.5 heights below the frame (160 x 120,
    cx = -2 w, cy = 2.5 h): the constant term cx * 20 / w of k_vote's approximate cell quotient is -40 and 50 cells, inside
    the range its error analysis covers (dh_vote_cell_fast_), so the fast path stays on.  Votes ON, and 1e-6 .. 1e-2 px beside,
    borders of the 20 x 20 guess grid; the emulated fast path agrees with the reference for every admissible reciprocal."""
    w, h = 160, 120
    K = synth.default_intrinsic(w, h)
    K[0, 2], K[1, 2] = -2.0 * w, 2.5 * h
    fx = float(K[0, 0])
    assert fx == int(fx) and w % 20 == 0 and h % 20 == 0
    frames = np.full((2, h, w), int(fx), dtype=np.uint16)
    frames[1, :, : w // 2] = 0
    eps = [0.0, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 3e-4, -3e-4, 1e-3, -1e-3, 1e-2]
    cw, ch = w / 20.0, h / 20.0
    offs = np.array([[(40 % cw) + 4 * (j % 3) + e, (40 % ch) + 4 * (j % 2) - e, 0.0] for j, e in enumerate(eps)], dtype=np.float32)
    _one_leaf_offsets_ok(offs)
    model = synth.ModelParams(stepwidth=4)
    p3 = window_points(K, model, frames[0])
    votes, ref, fast = vote_cells(K, w, h, p3, offs)
    for cells in fast:
        assert np.array_equal(cells[votes], ref[votes])
    # the votes' pixel positions x2 sit on and beside the cell borders
    x2 = (p3[:, None, 0] - offs[None, :, 0]) * K[0, 0] / (p3[:, None, 2] - offs[None, :, 2]) + K[0, 2]
    d = np.abs(x2 / cw - np.rint(x2 / cw)) * cw
    assert (d < 1e-6).any() and ((d > 5e-7) & (d < 2e-2)).sum() > 100

    def reach(results):
        assert np.array_equal(results[0]["pos_grid"], _pos_grid(votes, ref, 1000 // len(offs)))
        assert results[0]["pos_grid"].astype(np.int64).sum() > 0 and (results[1]["patch_flags"] == 0).any()
    return Family(_one_leaf_forest(offs), model, frames, K, reach=reach)


def principal_point_far_off_the_frame() -> Family:
    """A principal point about 100 frame widths left of a 160 x 120 frame (cx = -15918.38..., found by search), where the
    constant term of k_vote's approximate cell quotient is about -1990 cells and the quotient's rounding errors pass the
    1e-4 border band.  Offsets (drawn to put votes within 6e-4 of a cell border, kept where the emulation mis-cells them)
    send, under each of the three reciprocals within 1 ulp of 1 / nz, several votes of a flat frame to a different cell from
    the reference's x2 * 20 / w.  The host keeps such a K off the fast path (dh_vote_cell_fast_)."""
    w, h = 160, 120
    K = synth.default_intrinsic(w, h)
    K[0, 2] = np.float32(-15918.3837890625)
    fx, z = float(K[0, 0]), int(K[0, 0])
    cw = w / 20.0
    model = synth.ModelParams(stepwidth=4)
    frames = np.full((2, h, w), z, dtype=np.uint16)
    frames[1, :, : w // 2] = 0
    p3 = window_points(K, model, frames[0])
    # candidates: window i's vote lands at x2 = (nx / nz) fx + cx = k * cw + e, |e| < 6e-4 cells, |ox| about <= 20 px
    rs = np.random.RandomState(3)
    m = 600
    oz = rs.uniform(-0.1, 0.1, m).astype(np.float32)        # (nx moves by about cx * oz / fx)
    xw = p3[rs.randint(0, len(p3), m), 0].astype(F64)
    pix = xw * fx / z + float(K[0, 2])
    u = np.round((pix - rs.uniform(-20, 20, m)) / cw) + rs.uniform(-6e-4, 6e-4, m)
    ox = (xw - (u * cw - float(K[0, 2])) * (z - oz.astype(F64)) / fx).astype(np.float32)
    cand = np.stack([ox, rs.uniform(-10, 10, m).astype(np.float32), oz], axis=-1)
    votes, ref, fast = vote_cells(K, w, h, p3, cand)
    keep = set()
    for cells in fast:                                  # the 8 candidates that mis-cell most votes, per reciprocal
        bad = ((cells != ref) & votes).sum(axis=0)
        keep.update(int(j) for j in np.argsort(-bad, kind="stable")[:8] if bad[j] > 0)
    offs = cand[sorted(keep)]
    _one_leaf_offsets_ok(offs)
    valtoadd = 1000 // len(offs)
    grids = []
    for f in frames:
        votes, ref, fast = vote_cells(K, w, h, window_points(K, model, f), offs)
        for cells in fast:
            assert ((cells != ref) & votes).sum() >= 3, "the fast quotient mis-cells too few votes"
        grids.append(_pos_grid(votes, ref, valtoadd))
        assert all(not np.array_equal(_pos_grid(votes, cells, valtoadd), grids[-1]) for cells in fast)

    def reach(results):
        for r, g in zip(results, grids):             # pyref counts every vote in the reference's cell
            assert np.array_equal(r["pos_grid"], g)
    return Family(_one_leaf_forest(offs), model, frames, K, reach=reach)


def nonfinite_rotations() -> Family:
    """Rotations of NaN, +-inf and 1e300 in voting leaves: the trace of their covariance is NaN or inf, so `<= 400` is false
    and the leaf casts no rotation vote (prediction.rs:600); its position votes still count."""
    forest = synth.synth_forest(6, 8, synth.FOREST_SEED_BASE + 24)
    voting = np.flatnonzero(forest.leaf_prob > 0.5)
    kinds = [np.nan, np.inf, -np.inf, 1e300]
    touched = []
    for j, L in enumerate(voting[::3]):
        rb, re = int(forest.rot_begin[L]), int(forest.rot_begin[L + 1])
        if re - rb < 2:
            continue
        forest.rotations[rb + j % (re - rb), j % 3] = kinds[j % 4]
        with np.errstate(all="ignore"):
            tr = pyref.trace_of_cov(forest.rotations[rb:re], np.float64)
        assert not tr <= pyref.MAX_VARIANCE_ROT, tr
        touched.append(int(L))
    w, h = 160, 128
    frames = _frames(3, w, h, 90)

    def reach(results):
        assert _hits(results, touched) > 0
    return Family(forest, synth.ModelParams(stepwidth=4), frames, synth.default_intrinsic(w, h), reach=reach)


def zero_meanshift_iterations() -> Family:
    """meanshift_iterations = 0: the loops of meanshift.rs:328-407 never run; the pose is the initial guess."""
    forest = synth.synth_forest(6, 9, synth.FOREST_SEED_BASE + 25)
    w, h = 160, 128
    frames = _frames(2, w, h, 12)

    def reach(results):
        for r in results:
            assert r["ms_trace_mid"].shape[0] == 1 and r["ms_trace_rot"].shape[0] == 1
            assert np.array_equal(r["ms_trace_mid"][0], r["guess_mid"])
    return Family(forest, synth.ModelParams(stepwidth=4, meanshift_iterations=0), frames, synth.default_intrinsic(w, h), reach=reach)


def underflowing_kernel() -> Family:
    """A sigma so small that every kernel entry but the centre underflows to 0 (expf(-norm / 2 sigma^2), meanshift.rs:228-252):
    the mean shift only sees the cell it stands on, and stops (den == 0) as soon as that cell is empty."""
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)
    sigma = 1e-3
    k = pyref.build_kernel(20, np.float32(sigma))
    assert k[(10, 10, 10)] == 1.0 and sum(1 for v in k.values() if v == 0.0) == len(k) - 1
    w, h = 160, 128
    frames = _frames(2, w, h, 14)

    def reach(results):
        assert all(r["ms_trace_mid"].shape[0] <= 2 for r in results)
    return Family(forest, synth.ModelParams(stepwidth=4, gaussian_sigma=sigma), frames, synth.default_intrinsic(w, h), reach=reach)


def meanshift_dead_end() -> Family:
    """Every window votes the same two rotation cells, A = g + (-10, 9, 0) and B = g + (9, -10, 0) around the rotation guess g,
    with equal weight: the first step moves to the truncated mean g - (1, 1, 0), whose window [-10, 9] holds neither cell,
    so the denominator is 0 on the second step and the trace ends after one step (meanshift.rs:387-392)."""
    g = np.array([60, 60, 60])
    A, B = g + [-10, 9, 0], g + [9, -10, 0]

    def deg(bins):
        t = np.asarray(bins) - 60                                      # bin = (deg * 120 / 360) as i32 + 60
        return np.where(t >= 0, 3.0 * t + 1.5, 3.0 * t - 1.5)
    rotations = np.array([deg(A), deg(A), deg(B), deg(B)], dtype=np.float64)
    offsets = np.array([[5.0, -3.0, 10.0], [4.0, -2.0, 11.0]] * 2, dtype=np.float32)
    forest = _forest([~0, ~1], np.zeros(0, dtype=NODE_DTYPE), [1.0, 1.0], [2, 2], offsets, rotations)
    w, h = 160, 128
    frames = _frames(2, w, h, 16)
    # rot_guess g_r (radians): guess bin = ((g_r * 180 / 3.14159 + 180) * 120 / 360) as i32 -> 60 for g_r = 1.5 / 3 * pi / 180
    rot = np.tile(np.array([0.5 * 3.14159 / 180.0] * 3), (2, 1))
    model = synth.ModelParams(stepwidth=4, gaussian_sigma=8.0, meanshift_iterations=5)

    def reach(results):
        for r in results:
            assert r["guess_rot"].tolist() == g.tolist()
            cells = {tuple(c[:3]) for c in r["rot_cells"]}
            assert cells == {tuple(A), tuple(B)}, cells
            assert r["ms_trace_rot"].shape[0] == 2, r["ms_trace_rot"]   # one step, then den == 0
    return Family(forest, model, frames, synth.default_intrinsic(w, h), None, rot, reach=reach)


def is_pinhole(K) -> bool:
    K = np.asarray(K, dtype=np.float32)
    return bool(K[0, 1] == 0 and K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1)


def decoy_cameras(fam) -> np.ndarray:
    """One decoy camera per frame of a family (float32 [n, 3, 3]) for the camera-table tests: pinhole variants of a pinhole K
    with other fx, fy, cx and cy; perturbations of every entry of a dense K."""
    out = []
    for j in range(fam.frames.shape[0]):
        D = np.asarray(fam.K, dtype=np.float32).copy()
        s = 1.0 + 0.03 * (j + 1)
        if is_pinhole(D):
            D[0, 0] *= s; D[1, 1] /= s; D[0, 2] += 2.5 * (j + 1); D[1, 2] -= 1.5 * (j + 1)
        else:
            D *= np.float32(s)
            D[0, 1] += 0.25; D[1, 0] -= 0.125; D[2, 0] += 1e-3 * (j + 1)
        out.append(D)
    return np.stack(out).astype(np.float32)


FAMILIES = {f.__name__: f for f in (
    hand_forest, integer_thresholds, nonfinite_thresholds, blank_frames, no_window_frame, one_row_of_windows, guess_overrides,
    odd_patch_dense_intrinsic, window_means_at_the_gate, probabilities_outside_the_unit_interval, nonfinite_offset_votes,
    mixed_rectangles_on_reachable_differences, hundreds_of_equal_rotations, vote_cells_at_grid_borders, nonfinite_rotations,
    zero_meanshift_iterations, underflowing_kernel, meanshift_dead_end, principal_point_beside_the_frame,
    principal_point_far_off_the_frame)}


# ================================================================== sibling consumers: predict_mask, the 2-D Hough image
@dataclass
class AuxFamily:
    forest: Forest
    model: synth.ModelParams
    frames: np.ndarray
    K: np.ndarray
    reach: Callable[[list], None] = field(default=lambda results: None)   # on [{"mask", "votes", "sums"}] from oracle/pyref.py
    expect: dict = field(default_factory=dict)   # properties of the blurred image / argmax (oracle): see expectations()


def aux_results(fam):
    out = []
    for f in fam.frames:
        votes, sums = pyref.hough_votes(fam.forest, fam.model, f, fam.K)
        out.append(dict(mask=pyref.predict_mask(fam.forest, fam.model, f), votes=votes, sums=sums))
    return out


def expectations(fam, blurred, frames):
    """What `expect` claims about the blurred vote images (the oracle's or the kernels'): `saturates` -- some pixel clamps
    at 65535; `kernel_longer_than` -- the blur kernel has more taps than the frame has rows and columns; `all_equal` /
    `depth0_winner` -- frame indices whose blurred image is constant (the last pixel wins) / whose argmax pixel has depth 0."""
    from oracle import pyoracle
    e = fam.expect
    if e.get("saturates"):
        assert any((b == 65535).any() for b in blurred)
    if e.get("kernel_longer_than"):
        n, h, w = frames.shape
        assert pyoracle.gaussian_kernel(fam.model.gaussian_sigma).size > max(w, h)
    for i in e.get("all_equal", ()):
        assert (blurred[i] == blurred[i].flat[0]).all()
    for i in e.get("depth0_winner", ()):
        flat = blurred[i].reshape(-1)
        best = flat.size - 1 - int(np.argmax(flat[::-1]))              # the last maximum (prediction.rs:351-356)
        assert frames[i].reshape(-1)[best] == 0, (i, best)


def _leaf_hits(fam, results_unused=None):
    hits = set()
    for f in fam.frames:
        h, w = f.shape
        for _, _, ox, oy in pyref._windows(fam.model, w, h):
            ls = pyref._leafs(fam.forest, fam.model, f, ox, oy)
            if ls is not None:
                hits.update(ls)
    return hits


def _vote_limit_forest(seed) -> tuple[Forest, dict]:
    """Seven trees whose leaves sit at the limits of prediction.rs:805-808 (`prob >= 0.95`; `(255.0 * prob) as usize /
    offsets.len()`, then `as u16`): prob 0.95 and one ulp below it, 1.9, +inf (valtoadd 65535), 1e300 (usize::MAX / 3 ->
    0x5555), NaN (no vote), and 256 / 255 / 248 offsets (valtoadd 0 / 1 / 0).  Two trees split; tree 6 is a second +inf
    leaf whose one offset equals the first one's, so every window that reaches both adds 2 x 65535 to one pixel."""
    rs = np.random.RandomState(seed)
    nodes = np.zeros(2, dtype=NODE_DTYPE)
    nodes[0] = ((10, 10, 34, 34), (40, 40, 64, 64), 0.0, ~1, ~0)      # leaf 0 (1.9) if avg1 - avg2 > 0, else leaf 1 (+inf)
    nodes[1] = ((0, 30, 24, 54), (50, 30, 74, 54), 5.0, ~3, ~2)      # leaf 2 (1e300) / leaf 3 (NaN)
    leaves = [  # (prob, number of offsets, valtoadd)
        (1.9, 1, 484), (np.inf, 1, 65535), (1e300, 3, 0x5555), (np.nan, 2, None), (0.95, 2, 121),
        (np.nextafter(0.95, 0.0), 1, None), (1.0, 256, 0), (1.0, 255, 1), (0.97, 248, 0), (np.inf, 1, 65535)]
    n = [k for _, k, _ in leaves]
    offsets = np.concatenate([rs.uniform(-40, 40, (k, 3)) * [1, 1, 0.5] for k in n]).astype(np.float32)
    offsets[int(np.sum(n[:9]))] = offsets[int(np.sum(n[:1]))]          # leaf 9 votes where leaf 1 does
    rotations = np.zeros((int(np.sum(n)), 3))
    forest = _forest([~4, ~5, 0, 1, ~6, ~7, ~8, ~9], nodes, [p for p, _, _ in leaves], n, offsets, rotations)
    for L, (p, k, v) in enumerate(leaves):
        if v is not None:
            assert (pyref.as_usize(F64(F64(255.0) * F64(p))) // k) & 0xFFFF == v, (L, p, k)
    return forest, {L: v for L, (_, _, v) in enumerate(leaves)}


def aux_vote_limits() -> AuxFamily:
    """Votes past 65535 on one pixel (the u16 `+=` of prediction.rs:832 wraps), the valtoadd limits of _vote_limit_forest,
    mask values from NaN / inf means; sigma 0.3 makes the blur's centre tap > 1, so it clamps at 65535."""
    forest, vals = _vote_limit_forest(3)
    w, h = 160, 128
    frames = _frames(3, w, h, 81)
    model = synth.ModelParams(stepwidth=4, gaussian_sigma=0.3)

    def reach(results):
        top = max(max(int(v) for v in r["sums"].flat) for r in results)
        assert top > 65535, top
        assert sum(int(sum(1 for v in r["sums"].flat if v > 65535)) for r in results) > 0
        assert set(range(10)) <= _leaf_hits(AuxFamily(forest, model, frames, synth.default_intrinsic(w, h)))
        masks = np.stack([r["mask"] for r in results])
        assert (masks == 255).any()
    return AuxFamily(forest, model, frames, synth.default_intrinsic(w, h), reach=reach, expect={"saturates": True})


def aux_mask_wide_stride() -> AuxFamily:
    """predict_mask with a stride (30) larger than the patch (21 x 15), sized so that the stride squares of
    prediction.rs:884-897 are clipped at all four borders (x + i < step / 2 ..., x + i - step / 2 >= w ...).  Frame 0 is
    foreground everywhere, so every window writes its square."""
    forest = synth.synth_forest(5, 7, synth.FOREST_SEED_BASE + 26, patch=(21, 15))
    w, h = 143, 108
    model = synth.ModelParams(stepwidth=30, subimage_width=21, subimage_height=15)
    xs, ys = list(range(10, w - 11, 30)), list(range(7, h - 8, 30))
    half = 15
    assert xs[0] < half and ys[0] < half and xs[-1] + 30 - half > w and ys[-1] + 30 - half > h
    frames = _frames(3, w, h, 85)
    frames[0] = 900 + (np.arange(w * h).reshape(h, w) % 97)

    def reach(results):
        m = results[0]["mask"]
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
        assert (m > 0).all()
    return AuxFamily(forest, model, frames, synth.default_intrinsic(w, h), reach=reach)


def _aux_blur(w) -> AuxFamily:
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 170, n_frames=12, subset=1500)
    h = 96
    frames = _frames(2, w, h, 88)

    def reach(results):
        assert any(r["votes"].any() for r in results)
    return AuxFamily(forest, synth.ModelParams(stepwidth=4, gaussian_sigma=30.0), frames, synth.default_intrinsic(w, h),
                     reach=reach, expect={"kernel_longer_than": w < 121})


def aux_blur_w100() -> AuxFamily:
    """sigma 30: a 121-tap blur kernel on a 100 x 96 frame, longer than both sides (every tap position clamps)."""
    return _aux_blur(100)


def aux_blur_w255() -> AuxFamily:
    """Width one below the blur kernel's 256-thread tile."""
    return _aux_blur(255)


def aux_blur_w256() -> AuxFamily:
    """Width exactly one 256-thread tile."""
    return _aux_blur(256)


def aux_blur_w257() -> AuxFamily:
    """Width one past the 256-thread tile: a second tile with one live thread."""
    return _aux_blur(257)


def aux_argmax_ties() -> AuxFamily:
    """predict_parameter_from2dhough's argmax (prediction.rs:351-359): frame 0 casts no vote at all (its windows all take the
    no-vote leaf), so the blurred image is constant and the LAST pixel wins -- a pixel of depth 0; frame 1's votes are pushed
    off the head into the background, so its winner has depth 0 as well; frame 2 is an ordinary frame."""
    nodes = np.zeros(2, dtype=NODE_DTYPE)
    nodes[0] = nodes[1] = ((0, 0, 80, 80), (0, 0, 1, 1), 300.0, ~1, ~0)   # mean of the patch - its corner pixel > 300 -> voting leaf
    n = [6, 1]
    offsets = np.array([[-160, 0, 0], [-161, 1, 0], [-159, -1, 0], [-160, 2, 1], [-158, 0, -1], [-162, 1, 1], [0, 0, 0]], dtype=np.float32)
    forest = _forest([0, 1], nodes, [0.99, 0.5], n, offsets, np.zeros((7, 3)))
    w, h = 160, 128
    frames = _frames(3, w, h, 93)
    frames[0] = 500
    frames[0, -1, -1] = 0

    def reach(results):
        assert not results[0]["votes"].any() and results[1]["votes"].any()
    return AuxFamily(forest, synth.ModelParams(stepwidth=3, gaussian_sigma=2.0), frames, synth.default_intrinsic(w, h),
                     reach=reach, expect={"all_equal": (0,), "depth0_winner": (0, 1)})


AUX_FAMILIES = {f.__name__: f for f in (
    aux_vote_limits, aux_mask_wide_stride, aux_blur_w100, aux_blur_w255, aux_blur_w256, aux_blur_w257, aux_argmax_ties)}
