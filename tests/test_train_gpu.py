"""The trainer on the GPU (dh_trainer_*, depthhead_amd.training) against the C oracle tests/train_ref/train_oracle.c.
Every GPU forest here passes the oracle's node-by-node verifier (each split one of its node's regenerated candidates
and within 1e-12 of the best score, early_stop and comp_leaf_data bitwise, the negative-det count equal); where the
smallest best / second-best score gap is far above the last-ulp differences of the device's log (> 1e-9) the forest
also equals the oracle's own fit bit for bit.  Forests are deterministic and independent of how frames are split
across calls, predict through the existing path with oracle parity, and the edges of the contract hold."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_ref"))
import train_util as tu  # noqa: E402

from depthhead_amd import _lib, synth, training  # noqa: E402
from depthhead_amd._lib import DepthheadError  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = {
    "small": (dict(), (8, 96, 72)),
    "mid": (dict(stepwidth=6, W=32, H=32, max_depth=8, n_trees=4, subset=400, F=100, min_subset=10, seed=7), (16, 160, 120)),
    # 10 trees, depth 12, 48 frames of 320 x 240, 300 features, the trainer's 80 x 80 / 0.3 geometry
    "large": (dict(stepwidth=10, W=80, H=80, max_depth=12, n_trees=10, subset=1000, F=300, min_subset=20, seed=3), (48, 320, 240)),
}


def gpu_fit(p, chunks):
    with training.Trainer(p) as tr:
        for ch in chunks:
            tr.add_frames(*ch)
        return tr.fit(), tr.stats()


def split_chunks(data, parts):
    n = data[0].shape[0]
    cuts = np.linspace(0, n, parts + 1).astype(int)
    return [tuple(a[cuts[i]:cuts[i + 1]] for a in data) for i in range(parts)]


@pytest.fixture(scope="module")
def hip(hip_lib):
    return hip_lib


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_gpu_forest_equals_oracle_fit(hip, name):
    kw, (n, w, h) = CONFIGS[name]
    p = tu.params(**kw)
    data = tu.synthetic(n, w, h)
    ref, margin, neg = tu.oracle_train(p, [data])
    assert margin > 1e-9, f"fixture {name}: oracle margin {margin} too small for an exact comparison -- pick another seed"
    got, st = gpu_fit(p, [data])
    gap, vneg, _, _ = tu.oracle_verify(p, got)
    assert vneg == st["neg_det"] and gap == margin
    assert tu.forest_equal(got, ref), tu.forest_diff(got, ref)
    assert st["neg_det"] == neg
    lab, _, _ = tu.oracle_pool()
    assert st["pool_size"] == lab.size and st["pool_positives"] == int(lab.sum()) and st["frames"] == n
    assert sum(st["nodes_per_level"]) == got.n_nodes and sum(st["leaves_per_level"]) == got.n_leaves
    assert len(st["level_ms"]) == st["levels"] and all(x >= 0 for x in st["level_ms"])


def test_determinism_and_chunking(hip):
    kw, (n, w, h) = CONFIGS["mid"]
    p = tu.params(**kw)
    data = tu.synthetic(n, w, h)
    a, _ = gpu_fit(p, [data])
    b, _ = gpu_fit(p, [data])
    assert tu.forest_equal(a, b)
    c, _ = gpu_fit(p, split_chunks(data, 6))                  # one add_frames call and six give the same forest
    assert tu.forest_equal(a, c), tu.forest_diff(a, c)
    with training.Trainer(p) as tr:                            # fitting twice on one trainer
        tr.add_frames(*data)
        f1, f2 = tr.fit(), tr.fit()
    assert tu.forest_equal(f1, a) and tu.forest_equal(f2, a)
    p2 = tu.params(**dict(kw, seed=kw["seed"] + 1))
    d, _ = gpu_fit(p2, [data])
    assert not tu.forest_equal(a, d)


def test_end_to_end_prediction_parity_and_json(hip):
    from depthhead_amd.prediction import HoughPrediction, IntrinsicMatrix
    from depthhead_amd.stamm_json import export_json, import_json
    from oracle import pyoracle as po
    kw, (n, w, h) = CONFIGS["large"]
    hl = training.HoughLearning(kw["stepwidth"], kw["W"], kw["H"], kw["max_depth"], kw["n_trees"], kw["subset"], 0.3, kw["F"],
                                kw["min_subset"], 5.0, seed=kw["seed"])
    forest, model = hl.learn(8.0, training.synthetic_data(n, w, h))
    assert model.meanshift_iterations == 20 and model.stepwidth == kw["stepwidth"]
    ref, _, _ = tu.oracle_train(tu.params(**kw), [tu.synthetic(n, w, h)])
    assert tu.forest_equal(forest, ref), tu.forest_diff(forest, ref)
    errs = []
    with HoughPrediction(forest, model, device=0) as hp:
        for i in range(6):
            dep, mask, K, p3, rd = training.synthetic_truth(w, h, synth.FRAME_SEED_BASE + 1000 + i)   # held out
            pose = hp.predict_batch(dep[None], IntrinsicMatrix(K))
            r = po.predict(forest, model, dep, K)
            assert np.array_equal(pose["mid_point"][0], r.mid_point) and np.array_equal(pose["rotation"][0], r.rotation)
            errs.append(float(np.linalg.norm(pose["mid_point"][0].astype(np.float64) - p3)))
    # the oracle's fit of this set predicts the six held-out heads with a median error of 97.1 mm on the CPU
    assert np.median(errs) < 110.0, errs
    text = export_json(forest, model)
    back, mp = import_json(text, one_child="right")      # (the importer numbers nodes in its own order)
    assert export_json(back, mp) == text and back.n_leaves == forest.n_leaves


def _edge(p, data, chunks=1):
    """Verifier always; equality with the oracle's own fit where the score gap allows an exact comparison."""
    ref, margin, neg = tu.oracle_train(p, [data])
    got, st = gpu_fit(p, split_chunks(data, chunks))
    gap, vneg, _, _ = tu.oracle_verify(p, got)
    assert vneg == st["neg_det"]
    if margin > 1e-9:
        assert tu.forest_equal(got, ref), tu.forest_diff(got, ref)
        assert st["neg_det"] == neg
    return got


def test_default_parameters_verified(hip):
    """The trainer binary's defaults (20 trees, depth 15, 5200 samples, 2000 features, 80 x 80, 0.3) on 48 frames of
    640 x 480, no margin required: the first and the last tree through the verifier (about 7 s of oracle per tree)."""
    p = tu.params(stepwidth=10, W=80, H=80, max_depth=15, n_trees=20, subset=5200, scale=0.3, F=2000, min_subset=20, steep=5.0, seed=0)
    data = tu.synthetic(48, 640, 480)
    got, st = gpu_fit(p, [data])
    assert got.n_trees == 20 and got.max_depth() >= 10
    tu.oracle().to_reset()
    assert tu.oracle_add(p, *data) == 0
    for trees in ((0, 1), (19, 20)):
        gap, _, nodes, leaves = tu.oracle_verify(p, got, trees)
        assert nodes > 50 and leaves == nodes + 1, (trees, nodes, leaves)


def test_edge_no_positive(hip):
    fr, ma, K, p3, rd = tu.synthetic(4)
    got = _edge(tu.params(), (fr, np.zeros_like(ma), K, p3, rd))
    assert got.n_nodes == 0 and got.n_leaves == 3 and (got.roots < 0).all() and (got.leaf_prob == 0).all()
    assert got.offsets.shape[0] == 0


@pytest.mark.parametrize("kw", [dict(min_subset=500), dict(max_depth=0), dict(F=1), dict(scale=1.0), dict(scale=0.05),
                                dict(subset=2000), dict(W=21, H=19, stepwidth=5)])
def test_edges_match_oracle(hip, kw):
    data = tu.synthetic(6, 101, 77)                              # frame sizes off the stride
    got = _edge(tu.params(**kw), data, chunks=2)
    if "min_subset" in kw or "max_depth" in kw:
        assert got.n_nodes == 0 and got.n_leaves == 3
    if kw.get("scale") == 1.0:                                   # r1 == r2: no split leaves both sides non-empty
        assert got.n_nodes == 0
    if kw.get("scale") == 0.05:                                  # nw = 0.8: empty rectangles, every mean is 0, no split
        assert got.n_nodes == 0 and got.n_leaves == 3


def test_edge_one_empty_dimension(hip):
    """W = 3, H = 80 at 0.3: rectangles 0 x 24 (count 0 -> mean 0) on a non-square patch: every candidate compares
    0 - 0 with its threshold, so no split is valid and every tree is one leaf."""
    got = _edge(tu.params(W=3, H=80, stepwidth=3, scale=0.3), tu.synthetic(4, 120, 100), chunks=2)
    assert got.n_nodes == 0 and got.n_leaves == 3 and (got.leaf_prob > 0).all()


def test_edge_81x79_patch(hip):
    _edge(tu.params(W=81, H=79, stepwidth=7, scale=0.3, subset=300, max_depth=6), tu.synthetic(6, 203, 157), chunks=3)


def test_edge_frames_at_65535(hip):
    fr, ma, K, p3, rd = tu.synthetic(4, 96, 72)
    fr = np.where(fr > 0, 65535, 0).astype(np.uint16)
    fr[:, :, :8] = 65535
    _edge(tu.params(W=80, H=60, stepwidth=4), (fr, ma, K, p3, rd))


def test_edge_frames_smaller_than_patch(hip):
    data = tu.synthetic(2, 40, 30)
    with training.Trainer(tu.params(W=48, H=16)) as tr:
        with pytest.raises(DepthheadError) as e:
            tr.add_frames(*data)
        assert e.value.code == -5 and "smaller than" in str(e.value)


def test_invalid_inputs_rejected(hip):
    lib = _lib.load()
    h = C.c_void_p()
    for kw in (dict(scale=0.0), dict(scale=1.5), dict(F=0), dict(steep=0.0), dict(n_trees=0), dict(stepwidth=0)):
        assert lib.dh_trainer_create(C.byref(tu.params(**kw)), 0, C.byref(h)) == -1, kw
    assert lib.dh_trainer_create(C.byref(tu.params(W=300, H=300)), 0, C.byref(h)) == -5
    assert lib.dh_trainer_create(C.byref(tu.params()), 99, C.byref(h)) == -1
    with training.Trainer(tu.params()) as tr:
        f = C.c_void_p()
        assert lib.dh_trainer_fit(tr._h, C.byref(f)) == -6                  # empty pool
        assert lib.dh_trainer_add_frames(tr._h, None, None, 1, 96, 72, None, None, None) == -1
        assert lib.dh_trainer_add_frames(tr._h, None, None, -1, 96, 72, None, None, None) == -1
        st = tr.stats()
        assert st["pool_size"] == 0 and st["frames"] == 0
