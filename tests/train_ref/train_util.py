"""Test helpers for the trainer: the C oracle (train_oracle.c, built with gcc into a temp dir and loaded through ctypes)
and small synthetic training sets."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from depthhead_amd import _lib, training
from depthhead_amd.forest import NODE_DTYPE, Forest

HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        d = tempfile.mkdtemp(prefix="train_oracle_")
        so = os.path.join(d, "libtrain_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-std=c11",
                               os.path.join(HERE, "train_oracle.c"), "-o", so, "-lm"])
        lib = C.CDLL(so)
        lib.to_key.restype = C.c_uint64
        lib.to_key.argtypes = [C.c_uint64] * 4
        lib.to_pool_size.restype = C.c_size_t
        lib.to_impurity.restype = C.c_double
        lib.to_impurity.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_double]
        lib.to_cov_det.restype = C.c_double
        lib.to_cov_det.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        lib.to_scale_and_replace.argtypes = [C.c_uint32] * 4 + [C.c_double] * 3 + [C.c_void_p]
        lib.to_neg_det.restype = C.c_uint64
        lib.to_pool_set.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.to_pool_get.argtypes = [C.c_void_p] * 3
        lib.to_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.to_fit.argtypes = [C.c_void_p] * 11
        _ORACLE = lib
    return _ORACLE


def params(stepwidth=4, W=16, H=16, max_depth=5, n_trees=3, subset=200, scale=0.3, F=40, min_subset=5, steep=5.0, seed=1):
    return _lib.TrainParams(stepwidth, W, H, max_depth, n_trees, subset, scale, F, min_subset, steep, seed)


def _stack(data):
    fr, ma, K, p3, rd = zip(*data)
    return (np.ascontiguousarray(np.stack(fr), np.uint16), np.ascontiguousarray(np.stack(ma) != 0, np.uint8),
            np.ascontiguousarray(np.stack([np.asarray(k, np.float32).reshape(9) for k in K])),
            np.ascontiguousarray(np.stack(p3), np.float32), np.ascontiguousarray(np.stack(rd), np.float32))


def synthetic(n, w=96, h=72, first=0):
    return _stack(list(training.synthetic_truth(w, h, 0xD0E70000 + first + i) for i in range(n)))


def oracle_add(p, frames, masks, K, p3, rd):
    lib = oracle()
    n, h, w = frames.shape
    return lib.to_add(C.byref(p), frames.ctypes.data, masks.ctypes.data, n, w, h, K.ctypes.data, p3.ctypes.data, rd.ctypes.data)


def oracle_pool():
    lib = oracle()
    n = lib.to_pool_size()
    lab, off, rot = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float64)
    if n:
        lib.to_pool_get(lab.ctypes.data, off.ctypes.data, rot.ctypes.data)
    return lab, off, rot


def oracle_fit(p):
    """-> (Forest, margin, neg_det) from the pool currently held by the oracle."""
    lib = oracle()
    cap = p.n_trees * (2 * p.subset_per_tree + 1) + 1
    roots = np.zeros(p.n_trees, np.int32)
    nodes = np.zeros(cap, NODE_DTYPE)
    prob = np.zeros(cap, np.float64)
    ob, rb = np.zeros(cap + 1, np.uint32), np.zeros(cap + 1, np.uint32)
    offs = np.zeros((p.n_trees * p.subset_per_tree + 1, 3), np.float32)
    rots = np.zeros((p.n_trees * p.subset_per_tree + 1, 3), np.float64)
    counts = np.zeros(3, np.uint32)
    margin, neg = C.c_double(), C.c_uint64()
    rc = lib.to_fit(C.byref(p), roots.ctypes.data, nodes.ctypes.data, prob.ctypes.data, ob.ctypes.data, rb.ctypes.data,
                    offs.ctypes.data, rots.ctypes.data, counts.ctypes.data, C.byref(margin), C.byref(neg))
    assert rc == 0, rc
    nn, nl, nv = (int(x) for x in counts)
    f = Forest(roots, nodes[:nn], prob[:nl], ob[:nl + 1], rb[:nl + 1], offs[:nv], rots[:nv])
    return f, margin.value, neg.value


def oracle_train(p, data_chunks):
    oracle().to_reset()
    for ch in data_chunks:
        assert oracle_add(p, *ch) == 0
    return oracle_fit(p)


def forest_equal(a: Forest, b: Forest) -> bool:
    return (np.array_equal(a.roots, b.roots) and a.nodes.tobytes() == b.nodes.tobytes()
            and a.leaf_prob.tobytes() == b.leaf_prob.tobytes() and np.array_equal(a.off_begin, b.off_begin)
            and np.array_equal(a.rot_begin, b.rot_begin) and a.offsets.tobytes() == b.offsets.tobytes()
            and a.rotations.tobytes() == b.rotations.tobytes())


def forest_diff(a: Forest, b: Forest) -> str:
    for name in ("roots", "nodes", "leaf_prob", "off_begin", "rot_begin", "offsets", "rotations"):
        x, y = getattr(a, name), getattr(b, name)
        if x.shape != y.shape:
            return f"{name}: shape {x.shape} != {y.shape}"
        if x.tobytes() != y.tobytes():
            i = int(np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))[0]) if len(x) else 0
            return f"{name}[{i}]: {x[i]} != {y[i]}"
    return "equal"


def oracle_verify(p, f: Forest, trees=None):
    """Run the oracle's verifier over trees `trees` (default all) of `f` against the pool the oracle holds.
    -> (gap, neg_det, split nodes visited, leaves visited); raises AssertionError with the verifier's message."""
    lib = oracle()
    lib.to_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                              C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    t0, t1 = (0, f.n_trees) if trees is None else trees
    offs = np.ascontiguousarray(f.offsets if f.offsets.size else np.zeros((1, 3), np.float32))
    rots = np.ascontiguousarray(f.rotations if f.rotations.size else np.zeros((1, 3)))
    nodes = f.nodes if f.n_nodes else np.zeros(1, NODE_DTYPE)
    gap, neg = C.c_double(), C.c_uint64()
    visited = np.zeros(2, np.uint32)
    msg = C.create_string_buffer(512)
    rc = lib.to_verify(C.byref(p), f.roots.ctypes.data, nodes.ctypes.data, f.n_nodes, f.leaf_prob.ctypes.data,
                       f.off_begin.ctypes.data, f.rot_begin.ctypes.data, f.n_leaves, offs.ctypes.data, rots.ctypes.data, t0, t1,
                       C.byref(gap), C.byref(neg), visited.ctypes.data, msg, 512)
    assert rc == 0, msg.value.decode()
    if trees is None:
        assert visited[0] == f.n_nodes and visited[1] == f.n_leaves, (visited, f.n_nodes, f.n_leaves)
    return gap.value, neg.value, int(visited[0]), int(visited[1])


def _votes_equal_nan(x: np.ndarray, y: np.ndarray) -> bool:
    """Bitwise equal, except that a NaN matches any NaN at the same position."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    nx, ny = np.isnan(x), np.isnan(y)
    if not np.array_equal(nx, ny):
        return False
    u = np.uint32 if x.dtype == np.float32 else np.uint64
    return np.array_equal(x.view(u)[~nx], y.view(u)[~ny])


def forest_equal_nan(a: Forest, b: Forest) -> bool:
    """forest_equal with NaN-tolerant votes: the structure (roots, nodes, leaf probabilities, vote ranges) byte for byte,
    offsets and rotations bitwise except that NaN matches NaN (NaN bits are not part of the contract)."""
    return (np.array_equal(a.roots, b.roots) and a.nodes.tobytes() == b.nodes.tobytes()
            and a.leaf_prob.tobytes() == b.leaf_prob.tobytes() and np.array_equal(a.off_begin, b.off_begin)
            and np.array_equal(a.rot_begin, b.rot_begin) and _votes_equal_nan(a.offsets, b.offsets)
            and _votes_equal_nan(a.rotations, b.rotations))


def raw_add_frames(tr, frames, masks, K, p3, rd) -> int:
    """dh_trainer_add_frames on a training.Trainer with the arrays exactly as given (masks are not normalised to 0 / 1);
    -> the return code."""
    from depthhead_amd._lib import vp
    n, h, w = frames.shape
    arrs = (frames, masks, K, p3, rd)
    for a, dt, shape in zip(arrs, (np.uint16, np.uint8, np.float32, np.float32, np.float32),
                            ((n, h, w), (n, h, w), (n, 9), (n, 3), (n, 3))):
        assert a.dtype == dt and a.shape == shape and a.flags.c_contiguous, (a.dtype, a.shape)
    return tr._lib.dh_trainer_add_frames(tr._h, vp(frames), vp(masks), n, w, h, vp(K), vp(p3), vp(rd))


def oracle_run(p, calls):
    """Feed `calls` ((frames, masks, K, pos3d, rot_deg) each, masks as given) to a fresh oracle pool and fit it.
    -> (pool sizes after each call, Forest, margin, neg_det); the oracle keeps the pool (for oracle_verify)."""
    oracle().to_reset()
    sizes = []
    for ch in calls:
        assert oracle_add(p, *ch) == 0
        sizes.append(int(oracle().to_pool_size()))
    f, margin, neg = oracle_fit(p)
    return sizes, f, margin, neg
