"""k_traverse's gated tail (a tile runs the probability gate itself and lists only the windows that pass it; k_emit's pre-gated
instances read that list) against the path it replaces, the oracle, and the restatements of each request kind.  Every comparison is
byte for byte: the tail adds the same f64 leaf probabilities in the same order as k_emit does.

Geometry: 324 x 244, stride 4, DH_TILE=12,8 (96 windows a tile, 6 x 6 tiles), a fitted forest of 6 trees, batches of 19 frames (the
smallest that reach the tile lists) -- as in tests/test_gpu_tile_shift_families.py, whose frames these are.

(a) both paths, same bytes: poses, hit counts and the per-frame totals of gated windows with the gate in the tile and (DH_NO_TILE_GATE)
    in k_emit; the totals are the oracle's count of windows with patch flag 3;
(b) content at the edges of the rule, in one batch: an empty frame, noise that is gated nowhere, a frame whose every window is gated
    (full waves reserve list slots), a frame with exactly one gated window, windows whose leaf probabilities sum to 0.7 T (their mean
    is one ulp below the gate) and to the next f64 up (one ulp above);
(c) the rule's far side (several passes, taps, the general path, the guarded node table, a single-frame workspace) and near side
    (T * px * py = 4032 of 4096);
(d) state: big / small / big on one predictor, a replayed graph, forked sub-batches, a side stream;
(e) support, heads and a camera table under the gate; (f) cut tiles: DH_TILE_SHIFT=off and forced (8, 7).
"""
import dataclasses

import numpy as np
import pytest

import heads_ref as hr
import support_ref as sr
from depthhead_amd import synth
from test_gpu_tile_shift_families import (GEO, H, K0, MODEL, PX, PY, RADIUS, TILE, W, CachedOracle, _assert_poses, _device_call,
                                          _oracle_poses, env, kind_frames)

pytestmark = pytest.mark.gpu

F64 = np.float64
GATE = F64(0.7)


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import _lib, prediction, tracking
    return _lib, prediction, tracking


@pytest.fixture(scope="module")
def cached(oracle):
    return CachedOracle(oracle)


@pytest.fixture(scope="module")
def forest():
    return synth.fit_forest(6, 9, synth.FOREST_SEED_BASE + 83, n_frames=10, subset=1500)     # the forest of tests/test_gpu_tile_shift.py


@pytest.fixture(scope="module")
def tables(forest):
    return sr.LeafTables(forest)


@pytest.fixture(scope="module")
def frames():
    return kind_frames()


def _totals(results):
    """The oracle's count of windows that pass the probability gate (patch flag 3), per frame."""
    return np.array([int((r.patch_flags == 3).sum()) for r in results], np.uint32)


def _batch(prediction, forest, frs, model=MODEL, taps=False, **knobs):
    """(pose bytes, hit counts, gated windows per frame, tile_gate) of one batch on a fresh predictor under DH_TILE and the knobs."""
    knobs.setdefault("DH_TILE", TILE)
    with env(**knobs):
        with prediction.HoughPrediction(forest, model, device=0) as hp:
            if taps:
                hp.debug_enable(True)
            poses = hp.predict_batch(frs, prediction.IntrinsicMatrix(K0()))
            n = frs.shape[0]
            return poses, hp.debug_hit_counts(n), hp.debug_window_totals(n), hp.debug_geometry()["tile_gate"]


# ================================================================== (a) both paths, same bytes
def test_gate_in_the_tile_and_in_k_emit(mods, oracle, cached, forest, frames):
    _lib, prediction, _ = mods
    want = _oracle_poses(cached, forest, frames)
    on = _batch(prediction, forest, frames, DH_NO_TILE_GATE=None)
    off = _batch(prediction, forest, frames, DH_NO_TILE_GATE="1")
    assert on[3] is True and off[3] is False
    assert on[0].tobytes() == off[0].tobytes()
    assert np.array_equal(on[1], off[1]) and on[1].sum() > 0
    assert np.array_equal(on[2], _totals(want)) and np.array_equal(off[2], _totals(want))
    assert on[2].max() > 64 and (on[2] == 0).any()
    _assert_poses(on[0], want, "gate in the tile")


# ================================================================== (b) content at the edges of the rule
EMPTY, NOISE, FULL, ONE, ULP = 6, 7, 1, 3, 0       # slots of the content batch


def gate_sums(T):
    """(S0, S1): neighbouring f64 sums of T leaf probabilities on either side of the gate -- S0 the largest with fl(S0 / T) <= 0.7, S1
    the next f64 up, whose mean passes.  (Sums near 4.2 are 2^-50 apart, means near 0.7 2^-53: for T = 6 no sum divides to 0.7 itself;
    S0 = 6 x 0.7 rounded, its mean one ulp below 0.7, and the mean of S1 one ulp above.)"""
    s = F64(0.7) * F64(T)
    while F64(s / F64(T)) > GATE:
        s = np.nextafter(s, F64(0.0))
    while F64(np.nextafter(s, F64(8.0)) / F64(T)) <= GATE:
        s = np.nextafter(s, F64(8.0))
    return s, np.nextafter(s, F64(8.0))


def window_sums(prob, leaf_idx):
    """The sum of the leaf probabilities of every window: tree order, f64 (prediction.rs:582-584)."""
    s = np.zeros(leaf_idx.shape[0], F64)
    for t in range(leaf_idx.shape[1]):
        s = (s + prob[leaf_idx[:, t]]).astype(F64)
    return s


def content_frames(frames):
    f = np.array(frames)
    # a ramp: every window active, and the difference of two rectangle means depends on their offset alone, so every window reaches
    # the same leaf in a tree -- not the leaves of flat content, which noise reaches too
    f[FULL] = (100 + 12 * np.arange(W)[None, :] + 4 * np.arange(H)[:, None]).astype(np.uint16)
    assert f[EMPTY].max() == 0 and f[NOISE].min() > 0
    return f


def gated_by(prob, leaf_idx):
    return (window_sums(prob, leaf_idx) / F64(leaf_idx.shape[1])).astype(F64) > GATE


def content_forest(oracle, forest, f):
    """The fitted forest with leaf probabilities placed on the leaves these frames reach (the leaves a window reaches do not depend on
    them).  Leaves without votes keep 0 (the reference panics on a gated window that reaches a leaf with a probability and no vote);
    the others get 0.2; 0.9 on the five leaves with votes that the windows of the ramp reach; and 0.75 on: the leaves of two windows
    u, v of the subject frame ULP in their first five trees, with S0 - 3.75 / S1 - 3.75 in the last (3.75 = 5 x 0.75; both sums are
    exact in f64); the leaves of one window x of the subject frame ONE, chosen so that no other window of that frame passes."""
    T = forest.n_trees
    assert T == 6
    votes = (np.diff(forest.off_begin.astype(np.int64)) > 0) & (np.diff(forest.rot_begin.astype(np.int64)) > 0)
    base = {i: oracle.predict(forest, MODEL, f[i], K0()) for i in (FULL, ULP, ONE, NOISE)}
    flat = base[FULL].leaf_idx
    assert (flat == flat[0]).all() and votes[flat[0]].sum() == 5
    s0, s1 = gate_sums(T)
    assert F64(s0 / F64(T)) == np.nextafter(GATE, F64(0.0)) and F64(s1 / F64(T)) == np.nextafter(GATE, F64(1.0)) and s0 == F64(0.7) * F64(T)
    head = F64(0.75) * F64(T - 1)
    p0, p1 = F64(s0 - head), F64(s1 - head)
    assert F64(head + p0) == s0 and F64(head + p1) == s1 and 0.0 < p0 < p1 < 1.0

    def candidates(i, taken):
        li = base[i].leaf_idx[base[i].patch_flags > 0]
        return li[votes[li].all(axis=1) & ~np.isin(li, taken).any(axis=1)]
    cand = candidates(ULP, flat[0])
    u = cand[0]
    v = next(r for r in cand if r[T - 1] != u[T - 1] and u[T - 1] not in r[:T - 1] and r[T - 1] not in u[:T - 1])
    prob = np.where(votes, F64(0.2), F64(0.0))
    prob[flat[0][votes[flat[0]]]] = 0.9          # 5 x 0.9 / 6 = 0.75
    prob[u[:T - 1]] = 0.75
    prob[v[:T - 1]] = 0.75
    prob[u[T - 1]] = p0
    prob[v[T - 1]] = p1
    one = base[ONE].leaf_idx[base[ONE].patch_flags > 0]
    for x in candidates(ONE, np.concatenate([flat[0], u, v])):
        px = prob.copy()
        px[x] = 0.75
        if gated_by(px, one).sum() == 1:
            return dataclasses.replace(forest, leaf_prob=px), (s0, s1)
    raise AssertionError("no window of the frame ONE can be the only gated one")


def content_properties(results, prob, sums):
    """Each frame of the content batch has the property it is there for, from the oracle's flags and leaves."""
    flags = [np.asarray(r.patch_flags) for r in results]
    assert not flags[EMPTY].any(), "the empty frame has active windows"
    assert (flags[NOISE] == 1).all(), "noise: active everywhere, gated nowhere"
    assert (flags[FULL] == 3).all(), "the ramp: every window gated (every tile full, the cut ones too)"
    assert (flags[ONE] == 3).sum() == 1 and (flags[ONE] > 0).sum() > 300, "exactly one gated window (so: one in its tile)"
    act = flags[ULP] > 0
    s = window_sums(prob, np.asarray(results[ULP].leaf_idx)[act])
    below, above = s == sums[0], s == sums[1]
    assert below.any() and above.any(), "no window whose probabilities sum to 0.7 T / to the next f64 up"
    assert not (flags[ULP][act][below] == 3).any() and (flags[ULP][act][above] == 3).all()
    assert np.nextafter(sums[0], F64(8.0)) == sums[1]


def test_content_at_the_edges_of_the_rule(mods, oracle, forest, frames):
    _lib, prediction, _ = mods
    f = content_frames(frames)
    cf, sums = content_forest(oracle, forest, f)
    want = [oracle.predict(cf, MODEL, fr, K0()) for fr in f]
    content_properties(want, cf.leaf_prob, sums)
    tot = _totals(want)
    assert tot[EMPTY] == 0 and tot[NOISE] == 0 and tot[FULL] == GEO.nx * GEO.ny and tot[ONE] == 1
    ref = None
    for shift in ("off", None):
        on = _batch(prediction, cf, f, DH_TILE_SHIFT=shift, DH_NO_TILE_GATE=None)
        off = _batch(prediction, cf, f, DH_TILE_SHIFT=shift, DH_NO_TILE_GATE="1")
        assert on[3] is True and off[3] is False
        assert np.array_equal(on[2], tot) and np.array_equal(off[2], tot), shift
        assert np.array_equal(on[1], off[1])
        assert on[0].tobytes() == off[0].tobytes()
        ref = ref or on[0].tobytes()
        assert on[0].tobytes() == ref
        _assert_poses(on[0], want, f"shift {shift}")


# ================================================================== (c) the rule's far and near side
def _trees(n):
    return synth.synth_forest(n, 5, synth.FOREST_SEED_BASE + 0x91 + n)


@pytest.mark.parametrize("what,n_trees,taps,knobs,gated", [
    ("several passes", 43, False, {}, False),                  # 96 x 43 = 4128 > 4096
    ("one pass, just", 42, False, {}, True),                   # 96 x 42 = 4032
    ("taps", 0, True, {}, False),
    ("general path", 0, False, {"DH_FORCE_GENERAL": "1"}, False),
    ("guarded node table", 0, False, {"DH_NO_ABSORB": "1"}, False),
])
def test_sides_of_the_rule(mods, oracle, cached, forest, frames, what, n_trees, taps, knobs, gated):
    _lib, prediction, _ = mods
    assert PX * PY * 43 > 4096 >= PX * PY * 42
    fo = _trees(n_trees) if n_trees else forest
    frs = frames if not n_trees else np.ascontiguousarray(frames[[0, 6, 7, 3, 12, 16]])     # (the wide forests: six frames, no lists)
    want = [cached.predict(fo, MODEL, fr, K0()) for fr in frs]
    poses, hits, tot, tg = _batch(prediction, fo, frs, taps=taps, **knobs)
    assert tg is gated, what
    _assert_poses(poses, want, what)
    assert np.array_equal(tot, _totals(want)), what
    assert tot.sum() > 0


def test_single_frame_workspace_keeps_the_gate_in_k_emit(mods, oracle, cached, forest, frames):
    """A workspace of one frame serves latency, and the rule leaves it alone; grown to two frames the same predictor gates in the tile."""
    _lib, prediction, _ = mods
    with env(DH_TILE=TILE):
        with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
            for n, gated in ((1, False), (2, True)):
                frs = np.ascontiguousarray(frames[:n])
                want = _oracle_poses(cached, forest, frs)
                poses = hp.predict_batch(frs, prediction.IntrinsicMatrix(K0()))
                assert hp.debug_geometry()["tile_gate"] is gated
                assert np.array_equal(hp.debug_window_totals(n), _totals(want))
                _assert_poses(poses, want, f"{n} frame(s)")


# ================================================================== (d) state
def test_big_small_big_on_one_predictor(mods, oracle, cached, forest, frames):
    """A gated batch with lists, a 3-frame batch (no lists), the first batch rolled by 5 slots: totals and poses each time."""
    _lib, prediction, _ = mods
    batches = [np.ascontiguousarray(frames), np.ascontiguousarray(frames[3:6]), np.ascontiguousarray(np.roll(frames, 5, axis=0))]
    with env(DH_TILE=TILE):
        with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
            for k, frs in enumerate(batches):
                want = _oracle_poses(cached, forest, frs)
                poses = hp.predict_batch(frs, prediction.IntrinsicMatrix(K0()))
                assert hp.debug_geometry()["tile_gate"] is True
                assert np.array_equal(hp.debug_window_totals(frs.shape[0]), _totals(want)), f"batch {k}"
                _assert_poses(poses, want, f"batch {k}")


def test_graph_replayed_over_rewritten_frames(mods, oracle, cached, forest, frames):
    """One capture, three launches over frames rewritten in place (the batch, a permutation, its reverse with frame 0 emptied)."""
    import torch
    _lib, prediction, _ = mods
    n = frames.shape[0]
    dev = torch.device("cuda", 0)
    perm = np.random.RandomState(3).permutation(n)
    third = np.ascontiguousarray(frames[perm][::-1]).copy()
    third[0] = 0
    with env(DH_TILE=TILE):
        with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
            buf = torch.from_numpy(np.array(frames).view(np.int16)).to(dev)
            out = torch.zeros(n * _lib.POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            hp.reserve(n, W, H)
            hp.graph_capture(buf.data_ptr(), n, W, H, prediction.IntrinsicMatrix(K0()), out.data_ptr())
            st = torch.cuda.current_stream(dev)
            for k, frs in enumerate((np.array(frames), np.array(frames[perm]), third)):
                buf.copy_(torch.from_numpy(frs.view(np.int16)))
                hp.graph_launch(st.cuda_stream)
                torch.cuda.synchronize()
                want = _oracle_poses(cached, forest, frs)
                _assert_poses(np.frombuffer(out.cpu().numpy().tobytes(), dtype=_lib.POSE_DTYPE), want, f"launch {k}")
                assert np.array_equal(hp.debug_window_totals(n), _totals(want)), f"launch {k}"
            assert hp.debug_geometry()["tile_gate"] is True


def test_forked_sub_batches(mods, oracle, cached, forest, frames):
    """set_forking(2) on 35 frames: the second sub-batch starts at frame 17 with counters of its own."""
    import torch
    _lib, prediction, _ = mods
    n = 35
    idx = np.random.RandomState(n).permutation(n) % frames.shape[0]
    frs = np.ascontiguousarray(frames[idx])
    all_want = _oracle_poses(cached, forest, frames)
    want = [all_want[i] for i in idx]
    call = _device_call(torch, prediction, _lib, frs, torch.cuda.current_stream())
    with env(DH_TILE=TILE):
        with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
            hp.set_forking(2)
            raw = call(hp)
            assert hp.debug_geometry()["tile_gate"] is True
            assert np.array_equal(hp.debug_window_totals(n), _totals(want))
    _assert_poses(np.frombuffer(raw, dtype=_lib.POSE_DTYPE), want, "two sub-batches")


def test_side_stream(mods, oracle, cached, forest, frames):
    import torch
    _lib, prediction, _ = mods
    n = frames.shape[0]
    want = _oracle_poses(cached, forest, frames)
    call = _device_call(torch, prediction, _lib, frames, torch.cuda.Stream(device=torch.device("cuda", 0)))
    with env(DH_TILE=TILE):
        with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
            raw = call(hp)
            assert np.array_equal(hp.debug_window_totals(n), _totals(want))
    _assert_poses(np.frombuffer(raw, dtype=_lib.POSE_DTYPE), want, "side stream")


# ================================================================== (e) request kinds, (f) cut tiles
def _gate_on_and_off(prediction, forest, call, shift=None):
    """call(hp) -> bytes with the gate in the tile and in k_emit: the same bytes, returned."""
    out = []
    for knob, gated in ((None, True), ("1", False)):
        with env(DH_TILE=TILE, DH_TILE_SHIFT=shift, DH_NO_TILE_GATE=knob):
            with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
                out.append(call(hp))
                assert hp.debug_geometry()["tile_gate"] is gated
    assert out[0] == out[1]
    return out[0]


def test_support_records(mods, oracle, cached, forest, tables, frames):
    _lib, prediction, _ = mods
    n = frames.shape[0]
    want = np.zeros(n, dtype=_lib.SUPPORT_DTYPE)
    mids = np.zeros((n, 3), np.float32)
    mg, mask = sr.head_guesses(cached, forest, MODEL, frames, K0())
    for i in range(n):
        res, rec, _ = sr.support_ref(cached, tables, MODEL, frames[i], K0(), RADIUS, mg[i] if mask[i] & 1 else None)
        want[i], mids[i] = sr.as_record(rec, _lib.SUPPORT_DTYPE), res.mid_point

    def call(hp):
        poses, sup = hp.predict_batch_support(frames, prediction.IntrinsicMatrix(K0()), RADIUS, mg, None, mask)
        return poses.tobytes() + sup.tobytes()

    raw = _gate_on_and_off(prediction, forest, call)
    poses = np.frombuffer(raw[:n * _lib.POSE_DTYPE.itemsize], dtype=_lib.POSE_DTYPE)
    assert np.array_equal(poses["mid_point"], mids)
    assert raw[n * _lib.POSE_DTYPE.itemsize:] == want.tobytes()


def test_heads(mods, oracle, cached, forest, tables, frames):
    _lib, prediction, _ = mods
    n, mh = frames.shape[0], 2
    want_n = np.zeros(n, np.uint32)
    want = np.zeros((n, mh), dtype=_lib.HEAD_DTYPE)
    for i in range(n):
        k, kept, _, _, _ = hr.heads_ref(cached, tables, MODEL, frames[i], K0(), mh, RADIUS)
        want_n[i], want[i] = k, hr.as_records(k, kept, mh, _lib.HEAD_DTYPE)
    assert (want_n >= 2).sum() >= 1, want_n

    def call(hp):
        nh, heads = hp.predict_heads(frames, prediction.IntrinsicMatrix(K0()), mh, RADIUS)
        return nh.tobytes() + heads.tobytes()

    assert _gate_on_and_off(prediction, forest, call) == want_n.tobytes() + want.tobytes()


def test_camera_table(mods, oracle, cached, forest, frames):
    _lib, prediction, tracking = mods
    n = frames.shape[0]
    Ks = np.repeat(K0()[None].astype(np.float32), n, axis=0)
    for i in range(1, n, 2):
        Ks[i, 0, 0] *= 1.05 + 0.01 * i
        Ks[i, 1, 1] *= 1.05 + 0.01 * i
        Ks[i, 0, 2] += 2.0 * i
        Ks[i, 1, 2] -= 1.5 * i
    Ks[4, 0, 1] = 0.75; Ks[4, 1, 0] = -0.5; Ks[4, 2, 0] = 1e-4; Ks[4, 2, 2] = 1.001      # no pinhole

    def call(hp):
        with tracking.Cameras(Ks) as cams:
            return hp.predict_batch_cameras(frames, cams).tobytes()

    poses = np.frombuffer(_gate_on_and_off(prediction, forest, call), dtype=_lib.POSE_DTYPE)
    for i in range(n):
        want = cached.predict(forest, MODEL, frames[i], Ks[i])
        assert np.array_equal(poses["mid_point"][i], want.mid_point) and np.array_equal(poses["rotation"][i], want.rotation), f"frame {i}"


@pytest.mark.parametrize("shift", ["off", "8,7"])
def test_cut_tiles(mods, oracle, cached, forest, frames, shift):
    """The fixed grid (tiles cut at the right and bottom edge) and the grid shifted by (8, 7) windows (cut at the left and top too):
    cx * cy < px * py, so a tile's slots in LDS are fewer than its threads' windows."""
    _lib, prediction, _ = mods
    n = frames.shape[0]
    want = _oracle_poses(cached, forest, frames)

    def call(hp):
        poses = hp.predict_batch(frames, prediction.IntrinsicMatrix(K0()))
        shifts, _ = hp.debug_tile_shifts(n)
        assert (shifts == ((0, 0) if shift == "off" else (8, 7))).all()
        return poses.tobytes() + hp.debug_hit_counts(n).tobytes() + hp.debug_window_totals(n).tobytes()

    raw = _gate_on_and_off(prediction, forest, call, shift)
    _assert_poses(np.frombuffer(raw[:n * _lib.POSE_DTYPE.itemsize], dtype=_lib.POSE_DTYPE), want, shift)
    assert raw[-4 * n:] == _totals(want).tobytes()
