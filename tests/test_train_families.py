"""The training families of tests/train_ref/train_families.py without a GPU: every family reaches its edge on the C oracle's
pool and forest, the oracle's pool equals the Python restatement's (tests/train_ref/train_pyref.py) bit for bit, NaN
matched by position, after every call of the plan, and for the families small enough the two restatements grow the same
forest.  tests/test_gpu_train_edges.py holds the device trainer to the oracle on the same families."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "train_ref"))
import train_families as tf  # noqa: E402
import train_util as tu  # noqa: E402

from depthhead_amd.forest import NODE_DTYPE, Forest  # noqa: E402

_cache = {}


def family(name):
    """-> (family, oracle Run, pyref Trainer) of `name`, built once per session."""
    if name not in _cache:
        fam = tf.FAMILIES[name]()
        _cache[name] = (fam, tf.oracle_run(fam), tf.pyref_pool(fam))
    return _cache[name]


def _bits_equal_nan(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and tu._votes_equal_nan(x, y)


@pytest.mark.parametrize("name", sorted(tf.FAMILIES))
def test_family_reaches_its_edge(name):
    fam, run, py = family(name)
    if fam.exact:
        assert run.margin > 1e-9, f"{name}: oracle margin {run.margin} too small for an exact comparison -- pick another seed"
    fam.reach(run, py)


@pytest.mark.parametrize("name", sorted(tf.FAMILIES))
def test_oracle_pool_equals_pyref_pool(name):
    fam, run, py = family(name)
    assert run.lab.tolist() == py.lab
    assert _bits_equal_nan(run.off, np.asarray(py.off, np.float32).reshape(-1, 3))
    assert _bits_equal_nan(run.rot, np.asarray(py.rot, np.float64).reshape(-1, 3))
    frames = np.cumsum([c.n for c in fam.calls])
    assert run.sizes == [sum(1 for w in py.where if w[0] < n) for n in frames]
    assert run.sizes[-1] == len(py.lab)


def _pyref_forest(fit) -> Forest:
    roots, nodes, leaves = fit
    nd = np.zeros(len(nodes), NODE_DTYPE)
    for i, (r1, r2, th, cz, co) in enumerate(nodes):
        nd[i] = (r1, r2, th, cz, co)
    ob = np.cumsum([0] + [len(o) for _, o, _ in leaves]).astype(np.uint32)
    offs = np.asarray([v for _, o, _ in leaves for v in o], np.float32).reshape(-1, 3)
    rots = np.asarray([v for _, _, r in leaves for v in r], np.float64).reshape(-1, 3)
    return Forest(np.asarray(roots, np.int32), nd, np.asarray([p for p, _, _ in leaves], np.float64), ob, ob.copy(), offs, rots)


@pytest.mark.parametrize("name", tf.PYREF_FIT)
def test_oracle_forest_equals_pyref_forest(name):
    fam, run, py = family(name)
    with np.errstate(all="ignore"):
        ref = _pyref_forest(py.fit())
    assert tu.forest_equal_nan(run.forest, ref), tu.forest_diff(run.forest, ref)


def test_raw_masks_pool_equals_normalised_pool():
    fam, run, _ = family("raw_masks")
    assert (fam.calls[0].masks > 1).any()
    other = tf.oracle_run(tf.normalised(fam))
    assert other.lab.tobytes() == run.lab.tobytes() and other.off.tobytes() == run.off.tobytes()
    assert other.rot.tobytes() == run.rot.tobytes() and tu.forest_equal(other.forest, run.forest)


def test_nan_aware_forest_comparison():
    fam, run, _ = family("nonfinite_truth")
    f = run.forest
    assert tu.forest_equal_nan(f, f)
    g = Forest(f.roots, f.nodes, f.leaf_prob, f.off_begin, f.rot_begin, f.offsets.copy(), f.rotations.copy())
    nan = np.flatnonzero(np.isnan(g.offsets).ravel())[0]
    g.offsets.ravel().view(np.uint32)[nan] ^= 0x80000000                     # another NaN's bits: equal here, not bytewise
    assert tu.forest_equal_nan(f, g) and not tu.forest_equal(f, g)
    fin = np.flatnonzero(np.isfinite(g.offsets).ravel())[0]
    g.offsets.ravel()[fin] = np.nextafter(g.offsets.ravel()[fin], np.float32(np.inf))
    assert not tu.forest_equal_nan(f, g)
    h = Forest(f.roots, f.nodes, f.leaf_prob, f.off_begin, f.rot_begin, f.offsets.copy(), f.rotations.copy())
    h.offsets.ravel()[nan] = 0.0                                             # NaN against a number
    assert not tu.forest_equal_nan(f, h)
    # the oracle's verifier matches NaN votes the same way
    g.offsets.ravel()[fin] = f.offsets.ravel()[fin]
    tf.oracle_run(fam)
    tu.oracle_verify(fam.params, g)
    with pytest.raises(AssertionError, match="differs from its positive"):
        tu.oracle_verify(fam.params, h)


def test_capacity_restatement():
    assert tf.capacity_growths([240, 480, 1100, 3000, 3100]) == [(0, 0, 1024), (480, 1024, 3072), (3000, 3072, 7168)]
    assert tf.capacity_growths([5000]) == [(0, 0, 5000)]
    assert [tf.chunk_frames(w, h) for w, h in ((48, 40), (640, 480), (1280, 960))] == [256, 124, 31]
