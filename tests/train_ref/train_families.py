"""Adversarial training families shared by tests/test_train_families.py (CPU: the C oracle against the Python restatement
and the reach of every family) and tests/test_gpu_train_edges.py (the device trainer against the oracle).

Each family is a small seeded function returning a `TrainFamily`: the trainer parameters, a call plan (the
dh_trainer_add_frames calls, each with its own frames, masks exactly as the C ABI receives them, per-frame K, pos3d and
rot_deg), `exact` (the oracle's best / second-best margin allows a bit-for-bit forest comparison) and `reach(run, py)`,
which asserts on the oracle's pool and forest (`run`) and on the Python restatement's sample positions (`py`) that the
edge is actually hit, so that a family cannot quietly become harmless."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable

import numpy as np

import train_pyref
import train_util as tu
from depthhead_amd import training

F32 = np.float32


@dataclass
class Call:
    frames: np.ndarray    # uint16 [n, h, w]
    masks: np.ndarray     # uint8 [n, h, w], any values (not normalised)
    K: np.ndarray         # float32 [n, 9]
    pos3d: np.ndarray     # float32 [n, 3]
    rot_deg: np.ndarray   # float32 [n, 3]

    def arrays(self):
        return self.frames, self.masks, self.K, self.pos3d, self.rot_deg

    @property
    def n(self):
        return self.frames.shape[0]


@dataclass
class TrainFamily:
    params: object
    calls: list
    exact: bool
    reach: Callable = field(default=lambda run, py: None)
    learn: bool = False        # the device side runs HoughLearning.learn over the frames; `calls` is learn's flush plan


@dataclass
class Run:
    """The oracle's side of a family: pool sizes after each call, the pool, its fit."""
    sizes: list
    lab: np.ndarray
    off: np.ndarray
    rot: np.ndarray
    forest: object
    margin: float
    neg: int


def oracle_run(fam: TrainFamily) -> Run:
    """Leaves the family's pool in the oracle (for tu.oracle_verify)."""
    sizes, f, margin, neg = tu.oracle_run(fam.params, [c.arrays() for c in fam.calls])
    lab, off, rot = tu.oracle_pool()
    return Run(sizes, lab, off, rot, f, margin, neg)


def pyref_pool(fam: TrainFamily) -> train_pyref.Trainer:
    py = train_pyref.Trainer(fam.params)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in fam.calls:
            py.add(*c.arrays())
    return py


def chunk_frames(w, h):
    """dh_train_chunk_frames_ restated: frames per upload chunk of one add_frames call."""
    per = w * h * 3 + (w + 1) * (h + 1) * 4
    return max(1, min(256, (256 << 20) // per))


def capacity_growths(sizes):
    """trainer_reserve restated over the pool sizes seen after each single-chunk call: cap = max(need, 2 cap + 1024) when
    need exceeds cap.  -> [(resident samples, old cap, new cap)] per growth."""
    cap, prev, out = 0, 0, []
    for s in sizes:
        if s > cap:
            new = max(s, 2 * cap + 1024)
            out.append((prev, cap, new))
            cap = new
        prev = s
    return out


def windows(p, w, h):
    """iterate_subimage's centres (xs, ys) for frames of w x h."""
    lw, lh = p.subimage_width // 2, p.subimage_height // 2
    return (list(range(lw, w - (p.subimage_width - lw), p.stepwidth)), list(range(lh, h - (p.subimage_height - lh), p.stepwidth)))


def patch_sum(p, img, x, y):
    lw, lh = p.subimage_width // 2, p.subimage_height // 2
    return int(img[y - lh:y - lh + p.subimage_height, x - lw:x - lw + p.subimage_width].astype(np.int64).sum())


def forest_depths(f):
    """-> list of (depth, is_split) for every node and leaf of every tree, breadth-first."""
    out = []
    for r in f.roots:
        q = [(int(r), 0)]
        while q:
            ref, d = q.pop(0)
            out.append((d, ref >= 0))
            if ref >= 0:
                q += [(int(f.nodes["child_zero"][ref]), d + 1), (int(f.nodes["child_one"][ref]), d + 1)]
    return out


def _call(items, masks=None, K=None):
    d, m, k, p3, rd = zip(*items)
    masks = np.stack(m) if masks is None else masks
    K = np.stack([np.asarray(x, F32).reshape(9) for x in k]) if K is None else K
    return Call(np.ascontiguousarray(np.stack(d), np.uint16), np.ascontiguousarray(masks, np.uint8),
                np.ascontiguousarray(K, F32), np.ascontiguousarray(np.stack(p3), F32), np.ascontiguousarray(np.stack(rd), F32))


def _synth(n, w, h, first):
    return [training.synthetic_truth(w, h, 0x7A170000 + first + i) for i in range(n)]


def _head(w, h, cx, cy, r, z, wall, seed):
    """A disc head of radius r px (bulging towards the camera from z mm) in front of `wall` (scalar or [h, w] array), its
    mask, a pinhole K, the head centre in camera space and a seeded rotation."""
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (xx - cx) ** 2 + (yy - cy) ** 2
    inside = d2 < r * r
    depth = np.broadcast_to(np.asarray(wall, np.int64), (h, w)).copy()
    depth[inside] = (z - 4.0 * np.sqrt(r * r - d2[inside])).astype(np.int64)
    f = 0.875 * w
    K = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], F32)
    rng = np.random.RandomState(seed)
    p3 = np.array([(cx - w / 2) * z / f, (cy - h / 2) * z / f, z], F32)
    return depth.astype(np.uint16), inside.astype(np.uint8), K, p3, rng.uniform(-40, 40, 3).astype(F32)


def _textured_wall(w, h, base, span, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.RandomState(seed)
    a, b = rng.randint(3, 40, 2)
    return base + (xx * a + yy * b + (xx // 7) * (yy // 5) * 11) % span


# ------------------------------------------------------------------ families
def per_frame_intrinsics() -> TrainFamily:
    """Every frame its own K (focal lengths, principal point and a non-zero skew all differ), frame sizes differ across
    calls: a device that read one frame's inverse for every frame of a chunk changes the offsets."""
    calls = []
    for c, (w, h, n) in enumerate(((96, 72, 5), (120, 90, 4))):
        items = _synth(n, w, h, 16 * c)
        Ks = []
        for i in range(n):
            fx = 0.8 * w + 7.0 * i + 3.0 * c
            K = np.array([[fx, 0.75 + 1.5 * i, w / 2 + 3 * i - 4], [0, fx * (1.0 + 0.03 * (i + 1)), h / 2 - 2 * i + 1], [0, 0, 1]], F32)
            Ks.append(K.reshape(9))
        calls.append(_call(items, K=np.stack(Ks)))
    p = tu.params(seed=3)

    def reach(run, py):
        for c in calls:
            assert (c.K[:, 1] != 0).all() and len({k.tobytes() for k in c.K}) == c.n
        # the pool built when every frame of a call is given that call's frame 0 K
        same = [Call(c.frames, c.masks, np.ascontiguousarray(np.broadcast_to(c.K[:1], c.K.shape)), c.pos3d, c.rot_deg) for c in calls]
        tu.oracle_run(p, [c.arrays() for c in same])
        _, off0, _ = tu.oracle_pool()
        diff = np.flatnonzero((off0 != run.off).any(axis=1))
        frames = {py.where[i][0] for i in diff}
        assert {1, 2, 3, 4} <= frames and {6, 7, 8} <= frames, sorted(frames)   # every frame but each call's first
    return TrainFamily(p, calls, True, reach)


RAW_VALUES = (1, 7, 128, 255)


def raw_masks() -> TrainFamily:
    """Masks holding {0, 1, 7, 128, 255}, with mask pixels over background (all-zero-patch) windows, handed to the ABI as
    they are."""
    p = tu.params(seed=5)
    items = _synth(6, 96, 72, 100)
    masks = []
    for i, (d, m, _, _, _) in enumerate(items):
        yy, xx = np.mgrid[0:72, 0:96]
        raw = np.where(m != 0, np.asarray(RAW_VALUES, np.uint8)[(xx + 3 * yy + i) % 4], 0).astype(np.uint8)
        d[0:16, 0:16] = 0                   # window (8, 8): an all-zero patch under a mask of 255 / 7
        raw[0:16, 0:16] = 255 if i % 2 else 7
        masks.append(raw)
    call = _call(items, masks=np.stack(masks))

    def reach(run, py):
        vals = {int(call.masks[f, y, x]) for (f, x, y), lab in zip(py.where, run.lab) if lab}
        assert len(vals - {0, 1}) >= 2, vals
        bg = 0
        xs, ys = windows(p, 96, 72)
        for f in range(call.n):
            for y in ys:
                for x in xs:
                    bg += call.masks[f, y, x] != 0 and patch_sum(p, call.frames[f], x, y) == 0
        assert bg >= call.n, bg
    return TrainFamily(p, [call], True, reach)


def normalised(fam: TrainFamily) -> TrainFamily:
    """The same family with every mask replaced by its 0 / 1 normalisation."""
    calls = [Call(c.frames, np.ascontiguousarray(c.masks != 0, np.uint8), c.K, c.pos3d, c.rot_deg) for c in fam.calls]
    return TrainFamily(fam.params, calls, fam.exact)


def pool_growth() -> TrainFamily:
    """Sixteen calls of six frames: the pool crosses the capacity rule (1024, then 3072) with samples resident."""
    p = tu.params(W=8, H=8, stepwidth=2, seed=4)
    calls = [_call(_synth(6, 96, 72, 200 + 6 * k)) for k in range(16)]

    def reach(run, py):
        grown = [g for g in capacity_growths(run.sizes) if g[0] > 0]
        assert len(grown) >= 2, capacity_growths(run.sizes)
    return TrainFamily(p, calls, True, reach)


def _small_heads(n, w, h, first):
    out = []
    for i in range(n):
        rng = np.random.RandomState(first + i)
        wall = np.where(np.mgrid[0:h, 0:w][0] > h // 3, _textured_wall(w, h, 1800, 300, first + i), 0)
        out.append(_head(w, h, rng.randint(w // 4, 3 * w // 4), rng.randint(h // 4, 3 * h // 4), rng.randint(5, 9),
                         rng.randint(700, 1400), wall, first + i))
    return out


def chunked_call_frame_cap() -> TrainFamily:
    """One call of 257 small frames: two upload chunks at the 256-frame cap, the second holding one frame."""
    p = tu.params(W=8, H=8, stepwidth=4, seed=6)
    call = _call(_small_heads(257, 48, 40, 0x300))
    assert chunk_frames(48, 40) == 256

    def reach(run, py):
        frames = {w[0] for w in py.where}
        assert 0 in frames and 256 in frames
    return TrainFamily(p, [call], True, reach)


def chunked_call_size_limit() -> TrainFamily:
    """One call of 32 frames of 1280 x 960: chunks of 31 and 1 at the size-based limit."""
    p = tu.params(W=32, H=32, stepwidth=32, seed=2)
    items = []
    for i in range(32):
        rng = np.random.RandomState(0x400 + i)
        items.append(_head(1280, 960, rng.randint(300, 980), rng.randint(250, 710), rng.randint(90, 140), rng.randint(800, 1500),
                           _textured_wall(1280, 960, 2500, 400, i), 0x400 + i))
    call = _call(items)
    assert chunk_frames(1280, 960) == 31

    def reach(run, py):
        frames = {w[0] for w in py.where}
        assert 0 in frames and 30 in frames and 31 in frames
    return TrainFamily(p, [call], True, reach)


MIXED = ((70, 48, 40), (10, 64, 48))


def mixed_items():
    """HoughLearning.learn's input for mixed_sizes_learn: 70 frames of 48 x 40, then 10 of 64 x 48."""
    out = []
    for k, (n, w, h) in enumerate(MIXED):
        out += _small_heads(n, w, h, 0x500 + 100 * k)
    return out


def mixed_sizes_learn() -> TrainFamily:
    """learn over 80 frames with a size change after 70: flushed at 64 frames, at the size change and at the end."""
    p = tu.params(W=8, H=8, stepwidth=4, seed=8)
    items = mixed_items()
    calls = [_call(items[:64]), _call(items[64:70]), _call(items[70:])]

    def reach(run, py):
        assert len(items) > training._LEARN_BATCH and items[63][0].shape == items[64][0].shape != items[70][0].shape
        assert run.sizes[0] < run.sizes[1] < run.sizes[2]
    return TrainFamily(p, calls, True, reach, learn=True)


def sat_wraps() -> TrainFamily:
    """640 x 480 frames of a head before a wall at 50 000 - 65 535 mm: each frame sums to more than 2^32, so the summed-area
    table wraps."""
    p = tu.params(W=32, H=32, stepwidth=16, seed=9)
    items = []
    for i in range(3):
        rng = np.random.RandomState(0x600 + i)
        items.append(_head(640, 480, rng.randint(200, 440), rng.randint(150, 330), rng.randint(40, 70), rng.randint(900, 1300),
                           _textured_wall(640, 480, 50000, 15536, 0x600 + i), 0x600 + i))
    call = _call(items)

    def reach(run, py):
        assert all(int(fr.astype(np.int64).sum()) >= 1 << 32 for fr in call.frames)
        assert run.forest.n_nodes > 0
    return TrainFamily(p, [call], True, reach)


def patch_at_area_bound() -> TrainFamily:
    """W = H = 256, the largest accepted patch, on saturated backgrounds: a kept patch sums to nearly 2^32."""
    p = tu.params(W=256, H=256, stepwidth=4, seed=10)
    items = []
    for i in range(4):
        rng = np.random.RandomState(0x700 + i)
        items.append(_head(288, 272, rng.randint(136, 148), rng.randint(130, 138), rng.randint(7, 11), rng.randint(800, 1000),
                           65535, 0x700 + i))
    call = _call(items)

    def reach(run, py):
        assert max(int(s.sum()) for s in py.patches) >= 0.99 * 2 ** 32
        assert run.lab.sum() > 0 and (run.lab == 0).sum() > 0
    return TrainFamily(p, [call], True, reach)


def partial_keep() -> TrainFamily:
    """Frames with 1 - 19 windows of a class, a frame without a non-background window, a frame exactly W x H in its own
    call (no window), a frame W + 1 wide (one window column), and positives whose centre depth is 0."""
    p = tu.params(W=8, H=8, stepwidth=4, seed=11)
    w, h = 40, 32
    wall = _textured_wall(w, h, 1500, 60, 1)
    a = _head(w, h, 18, 14, 5, 900, wall, 1)                 # 4 positives, 44 negatives
    db = np.zeros((h, w), np.int64)
    db[8:24, 20:36] = wall[8:24, 20:36]
    db[12, 24] = 0                                            # centre (24, 12): a positive of depth 0
    db[16, 28] = 0
    mb = np.ones((h, w), np.uint8)
    for x, y in ((32, 24), (28, 24), (32, 20)):
        mb[y, x] = 0
    b = (db.astype(np.uint16), mb, a[2], np.array([12.5, -3.25, 950.0], F32), np.array([1, 2, 3], F32))
    c = (np.zeros((h, w), np.uint16), np.ones((h, w), np.uint8), a[2], a[3], a[4])
    d = _head(8, 8, 4, 4, 3, 900, 1500, 2)                   # exactly W x H
    e = _head(9, 20, 4, 8, 2, 900, _textured_wall(9, 20, 1500, 60, 3), 3)   # one window column
    calls = [_call([a, b, c]), _call([d]), _call([e])]

    def reach(run, py):
        per = {}
        for (f, x, y), lab in zip(py.where, run.lab):
            per.setdefault(f, [0, 0])[int(lab)] += 1
        assert per[0][0] == 20 and 1 <= per[0][1] <= 19, per
        assert 1 <= per[1][0] <= 19 and 1 <= per[1][1] <= 19, per
        assert 2 not in per and 3 not in per                       # no non-background window / no window at all
        assert run.sizes[1] == run.sizes[0] and run.sizes[2] > run.sizes[1]
        assert {x for f, x, y in py.where if f == 4} == {4} and per[4] == [2, 1], per
        zero = {(x, y): i for i, (f, x, y) in enumerate(py.where) if f == 1 and run.lab[i] and b[0][y, x] == 0}
        assert {(24, 12), (28, 16)} <= set(zero) and all((run.off[i] == -b[3]).all() for i in zero.values()), zero
    return TrainFamily(p, calls, True, reach)


def tiny_rectangles() -> TrainFamily:
    """W = H = 2 at scale 0.5: 1 x 1 split rectangles and a 2 x 2 rectangle-sum image, the patch's raw pixels.  Every
    corner is trunc(u * (2 - 1)) = 0, so both rectangles of a candidate coincide, no candidate is valid and every tree is
    one leaf holding its whole subset."""
    p = tu.params(W=2, H=2, stepwidth=2, scale=0.5, seed=12)
    call = _call(_synth(4, 48, 40, 300))

    def reach(run, py):
        f = run.forest
        assert f.n_nodes == 0 and f.n_leaves == p.n_trees and (f.leaf_prob > 0).all()
        assert int(p.subimage_width * p.subrect_feature_scale) == 1 and run.lab.sum() > 0
    return TrainFamily(p, [call], True, reach)


def tiny_rectangles_spread() -> TrainFamily:
    """W = H = 4 at scale 0.25: 1 x 1 rectangles at corners 0 - 2, so splits compare single pixels of the 4 x 4 image."""
    p = tu.params(W=4, H=4, stepwidth=2, scale=0.25, seed=12)
    call = _call(_synth(4, 48, 40, 300))

    def reach(run, py):
        f = run.forest
        assert f.n_nodes > 0
        for r in ("r1", "r2"):
            assert ((f.nodes[r][:, 2] - f.nodes[r][:, 0]) == 1).all() and ((f.nodes[r][:, 3] - f.nodes[r][:, 1]) == 1).all()
        assert (f.nodes["r1"][:, :2] != f.nodes["r2"][:, :2]).any(axis=1).all()
    return TrainFamily(p, [call], True, reach)


def block_boundary(F, seed) -> Callable[[], TrainFamily]:
    def fam() -> TrainFamily:
        """F around the 256-lane workgroup of k_train_score, 8 trees: several levels of many nodes."""
        p = tu.params(F=F, n_trees=8, max_depth=6, seed=seed)
        call = _call(_synth(8, 96, 72, 400))

        def reach(run, py):
            per_level = {}
            for d, split in forest_depths(run.forest):
                per_level[d] = per_level.get(d, 0) + split
            assert sum(v >= 8 for v in per_level.values()) >= 3, per_level
        return TrainFamily(p, [call], True, reach)
    fam.__name__ = f"block_boundary_F{F}"
    return fam


def deepest_tree() -> TrainFamily:
    """max_depth = 30 (DH_TRAIN_MAX_DEPTH), min_subset = 1: the oracle's trees reach depth 16 and more, where heap indices
    in the candidate keys pass 2^16."""
    p = tu.params(W=8, H=8, stepwidth=2, max_depth=30, min_subset=1, n_trees=3, subset=600, F=12, scale=0.4, seed=13)
    call = _call(_synth(8, 96, 72, 500))

    def reach(run, py):
        assert max(d for d, _ in forest_depths(run.forest)) >= 16
    return TrainFamily(p, [call], True, reach)


def _zero_r2_K(frame, mask, p, K):
    """K with its third row changed so that r[2] = (Kinv (x, y, 1))[2] is exactly 0 in f32 on a line of positive centres:
    with fx = K[0], fy = K[4], the row (0, fy / y0, 1) gives Kinv's third row (0, -q / y0, q), q = fx fy / det, so r[2]
    vanishes on the window row y0 when y0 is a power of two (the scaling by y0 is then exact); (fx / x0, 0, 1) likewise
    on the column x0.  -> (K, (axis, line)) for the line holding the most positive centres."""
    xs, ys = windows(p, frame.shape[1], frame.shape[0])
    pos = [(x, y) for y in ys for x in xs if mask[y, x] and patch_sum(p, frame, x, y) > 0 and frame[y, x] > 0]
    lines = [(sum(c[axis] == v for c in pos), axis, v) for axis in (0, 1) for v in (16, 32, 64) if v in (xs, ys)[axis]]
    cnt, axis, v = max(lines)
    assert cnt > 0, lines
    K2 = np.array(K, F32).reshape(3, 3).copy()
    K2[2] = (K2[0, 0] / F32(v), 0, 1) if axis == 0 else (0, K2[1, 1] / F32(v), 1)
    kinv = train_pyref.inv3(K2.reshape(9))
    for x, y in pos:
        if (x, y)[axis] == v:
            t = F32(x) * kinv[6]
            t = t + F32(y) * kinv[7]
            t = t + F32(1) * kinv[8]
            assert t == 0, (x, y, t)
    return K2.reshape(9), (axis, v)


def nonfinite_truth() -> TrainFamily:
    """NaN in one frame's pos3d, NaN in another's rotation, and a K whose third row gives r[2] = 0 on positive centres
    (offsets inf / NaN).  A forest holds these votes, so the trainer keeps them and the device and the oracle must agree.
    (+-inf rotations, which no forest can hold, are refused by dh_trainer_add_frames: UNVOTABLE_ROTATIONS.)"""
    p = tu.params(seed=14)
    items = _synth(6, 96, 72, 600)
    call = _call(items)
    call.pos3d[1, 0] = np.nan
    call.rot_deg[2] = (np.nan, 5.0, -7.5)
    call.K[3], (axis, line) = _zero_r2_K(call.frames[3], call.masks[3], p, call.K[3])

    def reach(run, py):
        assert any(f == 3 and (x, y)[axis] == line and run.lab[i] and not np.isfinite(run.off[i]).all() for i, (f, x, y) in enumerate(py.where))
        f = run.forest
        assert f.n_nodes > 0
        mixed = 0
        for L in range(f.n_leaves):
            o = f.offsets[f.off_begin[L]:f.off_begin[L + 1]]
            r = f.rotations[f.rot_begin[L]:f.rot_begin[L + 1]]
            fin = np.isfinite(o).all(axis=1) & np.isfinite(r).all(axis=1)
            mixed += fin.any() and not fin.all()
        assert mixed >= 1
    return TrainFamily(p, [call], True, reach)


FAMILIES = {f.__name__: f for f in (
    per_frame_intrinsics, raw_masks, pool_growth, chunked_call_frame_cap, chunked_call_size_limit, mixed_sizes_learn,
    sat_wraps, patch_at_area_bound, partial_keep, tiny_rectangles, tiny_rectangles_spread,
    *(block_boundary(F, 20 + i) for i, F in enumerate((255, 256, 257, 511, 512, 513))),
    deepest_tree, nonfinite_truth)}

# rot_deg values dh_trainer_add_frames refuses (a voting leaf's rotation bin (deg * 120 / 360) as i32 + 60 must lie in
# [0, 120) after one wrap, as dh_forest_create requires), and the nearest values it keeps
UNVOTABLE_ROTATIONS = (np.inf, -np.inf, 540.0, -543.0, 1e30)
VOTABLE_ROTATIONS = (np.nan, 539.75, -542.75, 0.0)

# families small enough for train_pyref's fit (a few seconds each)
PYREF_FIT = ("per_frame_intrinsics", "raw_masks", "partial_keep", "tiny_rectangles", "tiny_rectangles_spread", "nonfinite_truth")
