"""The device trainer (dh_trainer_*) on the training families of tests/train_ref/train_families.py, against the C oracle
(tests/train_ref/train_oracle.c).  Every call of a family's plan goes through the raw C ABI (masks as given); after each
call the device's pool size equals the oracle's; every tree passes the oracle's verifier with the device's negative-det
count; exact families give the oracle's forest bit for bit (NaN votes matched as NaN).  Also: raw masks against their 0 / 1
normalisation on the device, fit -> add_frames -> fit, and the refusals: n_trees * subset_per_tree >= 2^32, a patch of
more than 65 537 pixels, and rotations no forest can hold."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_ref"))
import train_families as tf  # noqa: E402
import train_util as tu  # noqa: E402

from depthhead_amd import _lib, training  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(hip_lib):
    return hip_lib


def device_plan(fam):
    """-> (forest, stats, pool size after each call) of the family's plan on the device."""
    sizes = []
    with training.Trainer(fam.params) as tr:
        for c in fam.calls:
            assert tu.raw_add_frames(tr, *c.arrays()) == 0
            sizes.append(tr.stats()["pool_size"])
        return tr.fit(), tr.stats(), sizes


def device_learn(fam, monkeypatch):
    """HoughLearning.learn over mixed_sizes_learn's frames; -> (forest, stats, frames per add_frames call)."""
    p = fam.params
    seen = []
    add = training.Trainer.add_frames

    def spy(self, frames, *rest):
        seen.append(int(np.asarray(frames).shape[0]))
        return add(self, frames, *rest)
    monkeypatch.setattr(training.Trainer, "add_frames", spy)
    hl = training.HoughLearning(p.stepwidth, p.subimage_width, p.subimage_height, p.max_depth, p.n_trees, p.subset_per_tree,
                                p.subrect_feature_scale, p.features_per_node, p.min_subset_size, p.steepness, seed=p.seed)
    forest, _ = hl.learn(8.0, tf.mixed_items())
    return forest, hl.last_stats, seen


def check_against_oracle(fam, got, st, run):
    """`run` = tf.oracle_run(fam), whose pool the oracle still holds."""
    gap, vneg, nodes, leaves = tu.oracle_verify(fam.params, got)
    assert vneg == st["neg_det"] and nodes == got.n_nodes and leaves == got.n_leaves
    assert st["pool_size"] == run.sizes[-1] and st["pool_positives"] == int(run.lab.sum())
    if fam.exact:
        assert run.margin > 1e-9, run.margin
        assert gap == run.margin
        assert tu.forest_equal_nan(got, run.forest), tu.forest_diff(got, run.forest)
        assert st["neg_det"] == run.neg


@pytest.mark.parametrize("name", sorted(tf.FAMILIES))
def test_family_on_device(hip, name, monkeypatch):
    fam = tf.FAMILIES[name]()
    if fam.learn:
        got, st, seen = device_learn(fam, monkeypatch)
        assert seen == [c.n for c in fam.calls], seen           # flushed at 64 frames, at the size change, at the end
        sizes = None
    else:
        got, st, sizes = device_plan(fam)
    run = tf.oracle_run(fam)
    if sizes is not None:
        assert sizes == run.sizes, (sizes, run.sizes)
    assert st["frames"] == sum(c.n for c in fam.calls)
    check_against_oracle(fam, got, st, run)
    if name == "pool_growth":                                   # the capacity rule, restated over the observed pool sizes
        assert len([g for g in tf.capacity_growths(sizes) if g[0] > 0]) >= 2


def test_raw_masks_equal_normalised_on_device(hip):
    fam = tf.raw_masks()
    assert (fam.calls[0].masks > 1).any()
    a, sa, _ = device_plan(fam)
    b, sb, _ = device_plan(tf.normalised(fam))
    assert tu.forest_equal(a, b), tu.forest_diff(a, b)
    assert sa["pool_size"] == sb["pool_size"] and sa["pool_positives"] == sb["pool_positives"] and sa["neg_det"] == sb["neg_det"]
    with training.Trainer(fam.params) as tr:                  # the Python wrapper normalises; same forest again
        tr.add_frames(*fam.calls[0].arrays())
        assert tu.forest_equal(tr.fit(), a)


def test_fit_add_fit_matches_oracle_on_the_union(hip):
    kw = dict(stepwidth=6, W=32, H=32, max_depth=8, n_trees=4, subset=400, F=100, min_subset=10, seed=7)
    p = tu.params(**kw)
    first, second = tu.synthetic(10, 160, 120), tu.synthetic(6, 160, 120, first=10)
    ref1, m1, _ = tu.oracle_train(p, [first])
    ref, margin, neg = tu.oracle_train(p, [first, second])
    assert m1 > 1e-9 and margin > 1e-9, (m1, margin)
    with training.Trainer(p) as tr:
        tr.add_frames(*first)
        f1 = tr.fit()
        tr.add_frames(*second)
        f2 = tr.fit()
        st = tr.stats()
    assert tu.forest_equal(f1, ref1), tu.forest_diff(f1, ref1)
    assert tu.forest_equal(f2, ref), tu.forest_diff(f2, ref)
    assert st["neg_det"] == neg and st["frames"] == 16 and st["pool_size"] == tu.oracle().to_pool_size()
    assert not tu.forest_equal(f1, f2)


def test_tree_subset_product_refused(hip):
    """n_trees * subset_per_tree >= 2^32 overflows the level's u32 sample ranges: dh_trainer_fit refuses it with -5 on a
    small pool, before any level runs."""
    lib = _lib.load()
    data = tu.synthetic(2)
    for n_trees, subset in ((65537, 65536), (65536, 65536), (2, 0xFFFFFFFF)):
        with training.Trainer(tu.params(n_trees=n_trees, subset=subset)) as tr:
            tr.add_frames(*data)
            pool = tr.stats()["pool_size"]
            f = C.c_void_p()
            assert lib.dh_trainer_fit(tr._h, C.byref(f)) == -5 and not f.value
            st = tr.stats()
            assert st["levels"] == 0 and st["pool_size"] == pool > 0


def test_unvotable_rotations_refused(hip):
    """A rot_deg no forest can hold as a vote (dh_forest_create's one-wrap bin rule) is refused by add_frames with -1 and
    nothing added; the nearest values it keeps, NaN included, give a forest (which fit would otherwise fail to build)."""
    p = tu.params()
    fr, ma, K, p3, rd = tu.synthetic(3)
    with training.Trainer(p) as tr:
        assert tu.raw_add_frames(tr, fr[:1], ma[:1], K[:1], p3[:1], rd[:1]) == 0
        st0 = tr.stats()
        for v in tf.UNVOTABLE_ROTATIONS:
            bad = rd.copy()
            bad[2, 1] = v
            assert tu.raw_add_frames(tr, fr, ma, K, p3, bad) == -1, v
            assert "outside what a forest can hold" in _lib.load().dh_last_error().decode()
            st = tr.stats()
            assert st["pool_size"] == st0["pool_size"] and st["frames"] == st0["frames"] == 1, v
        ok = rd[1:].copy()
        ok[:, 0] = tf.VOTABLE_ROTATIONS[:2]
        ok[:, 2] = tf.VOTABLE_ROTATIONS[2:]
        assert tu.raw_add_frames(tr, fr[1:], ma[1:], K[1:], p3[1:], ok) == 0
        got, st = tr.fit(), tr.stats()
    calls = [(fr[:1], ma[:1], K[:1], p3[:1], rd[:1]), (fr[1:], ma[1:], K[1:], p3[1:], ok)]
    _, ref, margin, neg = tu.oracle_run(p, calls)
    tu.oracle_verify(p, got)
    assert margin > 1e-9 and tu.forest_equal_nan(got, ref), tu.forest_diff(got, ref)
    assert np.isnan(got.rotations).any() and st["neg_det"] == neg


def test_area_bound_refusal(hip):
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dh_trainer_create(C.byref(tu.params(W=198, H=331)), 0, C.byref(h)) == -5 and not h.value   # 65 538 pixels
    assert lib.dh_trainer_create(C.byref(tu.params(W=256, H=256)), 0, C.byref(h)) == 0 and h.value
    assert lib.dh_trainer_destroy(h) == 0
