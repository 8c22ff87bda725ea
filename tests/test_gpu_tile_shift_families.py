"""The per-frame shift of k_traverse's tile grid (k_tile_shift) held to every stride, rectangle, k_boxsum instance, mask block height,
copy path and request kind -- not only the one geometry of tests/test_gpu_tile_shift.py.  Every comparison is byte for byte.

(a) geometry families: one row per branch of dh_tile_shifts_ / k_traverse / k_boxsum that a non-zero shift has to get right;
(b) request kinds on the geometry of tests/test_gpu_tile_shift.py: support, heads, camera tables, guesses, the device forms, forked
    sub-batches, a replayed graph;
(c) state that survives a batch on one predictor (sparse-store masks, list lengths);
(d) the LDS limit of k_tile_shift's table, on either side.

The expected shifts and list lengths come from tests/tile_shift_ref.py, the expected outputs from the oracle and the restatements
the project already has for each kind (tests/support_ref.py, tests/heads_ref.py).  DESIGN.md section 10 lists which branch each row reaches.
"""
import contextlib
import os

import numpy as np
import pytest

import heads_ref as hr
import support_ref as sr
import tile_shift_ref as tsr
from depthhead_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import _lib, prediction, tracking
    return _lib, prediction, tracking


@contextlib.contextmanager
def env(**kv):
    """Knobs for the predictors created inside (the environment is read once, at creation); None leaves / makes a knob unset."""
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class CachedOracle:
    """The oracle with each frame's result computed once: the same frames run under several knobs."""

    def __init__(self, oracle):
        self._o, self._memo = oracle, {}

    def predict(self, forest, model, img, K, midp_guess=None, rot_guess=None, **kw):
        key = (id(forest), model.stepwidth, model.subimage_width, model.subimage_height, np.asarray(img).tobytes(), np.asarray(K, np.float32).tobytes(),
               None if midp_guess is None else np.asarray(midp_guess, np.float32).tobytes(),
               None if rot_guess is None else np.asarray(rot_guess, np.float64).tobytes())
        if key not in self._memo:
            self._memo[key] = self._o.predict(forest, model, img, K, midp_guess, rot_guess, **kw)
        return self._memo[key]


@pytest.fixture(scope="module")
def cached(oracle):
    return CachedOracle(oracle)


# ================================================================== (a) geometry families
# name: stride, frame, DH_TILE, patch, rect_scale, frames of the batch, workspace reserved (0 = the batch), further knobs, (trees, depth)
def _row(step, w, h, tile, patch=(80, 80), scale=0.3, n=15, reserve=0, knobs=None, trees=(6, 9)):
    return dict(step=step, w=w, h=h, tile=tile, patch=patch, scale=scale, n=n, reserve=reserve, knobs=knobs or {}, trees=trees)


FAMILIES = {
    "stride1": _row(1, 324, 244, (32, 24), n=10, trees=(2, 8)),      # lg 0
    "stride2": _row(2, 324, 244, (20, 14), n=13, trees=(3, 9)),      # lg 1
    "stride3": _row(3, 324, 244, (16, 12), n=18),                    # lg 0, odd stride
    "stride6": _row(6, 324, 244, (8, 6), n=18),                      # lg 1, step / m = 3
    "stride8": _row(8, 300, 250, (8, 3), n=17),                      # lg 3, gx 4
    "stride16": _row(16, 420, 250, (4, 2)),                          # lg 3, gx 2: sx = 2
    "stride32": _row(32, 600, 404, (4, 2), n=18),                    # lg 3, gx 1: sx in 0 .. 3
    "rect21": _row(4, 324, 244, (12, 8), scale=0.27),                # rw % 4 != 0: k_boxsum without the 16-byte read-back
    "rect32": _row(4, 324, 244, (12, 8), scale=0.4),                 # rh - 1 > 28: k_boxsum re-reads the leaving row
    "patch100x80": _row(4, 324, 244, (12, 8), patch=(100, 80), n=18),    # rectangle 30 x 24, tbw != tbh
    "width322": _row(4, 322, 244, (12, 8)),                          # w % 4 != 0: k_boxsum with 2-byte loads
    "parts1": _row(4, 252, 244, (8, 8)),                             # one k_boxsum part per band
    "parts3": _row(4, 520, 244, (20, 8)),                            # three
    "blocks16": _row(4, 324, 244, (12, 8), reserve=64),              # 16-row mask blocks
    "tile10": _row(4, 324, 244, (10, 8), n=13),                      # px % 4 != 0: cut tiles copied element by element
    "no_ring": _row(4, 324, 244, (12, 8), knobs={"DH_BOX_NO_RING": "1"}),   # the re-read instance by knob
    "one_frame": _row(1, 324, 245, None, n=1, trees=(40, 5)),        # single-frame workspace: one-pass tiles of 40 x 2 windows
}
ONE_FRAME_TILE = (40, 2)      # what the tile chooser gives one frame of 244 x 165 windows and 40 trees (asserted from debug_geometry)


def _geometry(row):
    rect = (int(row["patch"][0] * row["scale"]), int(row["patch"][1] * row["scale"]))
    return tsr.Geometry(row["w"], row["h"], row["step"], row["patch"], rect, row["tile"] or ONE_FRAME_TILE)


def _blob(f, geo, x0, y0, x1, y1):
    f[max(y0, 0):min(y1, geo.h), max(x0, 0):min(x1, geo.w)] = 900


def family_frames(geo, n, seed=8):
    """n >= 10 frames: subjects, an empty frame, an all-noise frame, a blob in each corner, and blobs whose rectangle sums begin
    exactly on a tile border of the unshifted grid, begin on one of the grid under its largest shift, and end on the last column
    and row before a border.  (The rectangle with origin (x, y) sums pixels [x, x + rw) x [y, y + rh): pixels from column c on make
    the sums non-zero from c - rw + 1 on, pixels up to column c make them non-zero up to c.)"""
    w, h, step = geo.w, geo.h, geo.step
    f = synth.biwi_batch(n, w, h, first=600)
    rs = np.random.RandomState(seed)
    f[1] = 0
    f[2] = rs.randint(400, 1400, (h, w)).astype(np.uint16)
    bw, bh = min(90, w // 3), min(70, h // 3)
    for i, (x0, y0) in enumerate(((0, 0), (w - bw, 0), (0, h - bh), (w - bw, h - bh))):
        f[3 + i] = 0
        _blob(f[3 + i], geo, x0, y0, x0 + bw, y0 + bh)
    tpx, tpy = geo.px * step, geo.py * step
    sx, sy = geo.largest_shift()
    f[7] = 0
    _blob(f[7], geo, tpx + geo.rw - 1, tpy + geo.rh - 1, tpx + geo.rw - 1 + 110, tpy + geo.rh - 1 + 90)
    f[8] = 0                                # tile (1, 1) of the grid shifted by (sx, sy) begins at window (px - sx, py - sy)
    _blob(f[8], geo, tpx - sx * step + geo.rw - 1, tpy - sy * step + geo.rh - 1, tpx - sx * step + geo.rw - 1 + geo.tbw - 1, tpy - sy * step + geo.rh - 1 + geo.tbh - 1)
    f[9] = 0
    kx, ky = max(2, min(3, geo.tiles_x - 1)), max(2, min(3, geo.tiles_y - 1))
    _blob(f[9], geo, kx * tpx - 44, ky * tpy - 36, kx * tpx, ky * tpy)
    return f


def one_frame(geo):
    """The single frame of the one-frame row: a top-left corner blob (the tiles a shift cuts) and a blob whose sums begin on a border of
    the grid under its largest shift."""
    f = np.zeros((1, geo.h, geo.w), np.uint16)
    _blob(f[0], geo, 0, 0, 30, 24)
    sx, sy = geo.largest_shift()
    x, y = (3 * geo.px - sx) * geo.step + geo.rw - 1, (40 * geo.py - sy) * geo.step + geo.rh - 1
    _blob(f[0], geo, x, y, x + 30, y + 21)
    return f


def family_case(name):
    """(row, geometry, frames, mask block height) of a family."""
    row = FAMILIES[name]
    geo = _geometry(row)
    frames = one_frame(geo) if row["n"] == 1 else family_frames(geo, row["n"])
    return row, geo, frames, geo.block(row["reserve"] or row["n"])


def family_expectations(name, case=None):
    """What the restatement says of a family: per frame (tiles at (0, 0), chosen shift, its tiles), the largest shift, the flag maps
    under it.  Asserts what the case needs to mean anything: the lists are on, frames choose, one chooses a non-zero shift, and the
    forced run walks a tile cut at the left edge and one cut at the top."""
    row, geo, frames, block = case or family_case(name)
    assert frames.shape[0] * geo.tiles > 512, "the batch runs without tile lists"
    assert geo.chooses(block), "no slack, or the table does not fit"
    ref, _ = tsr.choice(frames, geo, block)
    big = geo.largest_shift()
    maps = tsr.forced_counts(frames, geo, block, *big)
    assert any(s != (0, 0) for _, s, _ in ref), "no frame chooses a shift"
    assert big[0] > 0 and any(m[:, 0].any() for m in maps), "no flagged tile cut at the left edge"
    assert big[1] > 0 and any(m[0, :].any() for m in maps), "no flagged tile cut at the top"
    return ref, big, maps


def _run(prediction, forest, model, row, frames, shift):
    """Poses, shifts, list counts and the geometry of one batch on a fresh predictor; shift: None (automatic), "off" or "sx,sy"."""
    w, h = row["w"], row["h"]
    tile = None if row["tile"] is None else "%d,%d" % row["tile"]
    with env(DH_TILE=tile, DH_TILE_SHIFT=shift, **row["knobs"]):
        with prediction.HoughPrediction(forest, model, device=0) as hp:
            if row["reserve"]:
                hp.reserve(row["reserve"], w, h)
            poses = hp.predict_batch(frames, prediction.IntrinsicMatrix(synth.default_intrinsic(w, h)))
            shifts, counts = hp.debug_tile_shifts(frames.shape[0])
            geo = hp.debug_geometry()
    return poses, shifts, counts, geo


@pytest.mark.parametrize("name", list(FAMILIES))
def test_geometry_family(mods, oracle, cached, name):
    """DH_TILE_SHIFT unset, "off" and forced to the largest allowed shift: the product-mode taps and the poses equal the oracle, the
    pose bytes are the same in all three, the shifts and the list lengths are the restatement's.

    one_frame: 40 shallow trees rather than 50 -- with 50 the one-pass tile is 64 x 1 windows, whose grid has no slack in y and so
    no tile cut at the top; with 40 it is 40 x 2 (7 x 83 = 581 tiles: one frame reaches the lists)."""
    from test_gpu_round2 import _product_mode_check
    _, prediction, _ = mods
    row, geo, frames, block = family_case(name)
    ref, big, maps = family_expectations(name, (row, geo, frames, block))
    model = synth.ModelParams(stepwidth=row["step"], subimage_width=row["patch"][0], subimage_height=row["patch"][1])
    forest = synth.synth_forest(*row["trees"], synth.FOREST_SEED_BASE + 0x75 + row["step"], patch=row["patch"], rect_scale=row["scale"])
    K = synth.default_intrinsic(row["w"], row["h"])
    n = frames.shape[0]

    runs = {}
    for mode, shift in (("auto", None), ("off", "off"), ("forced", "%d,%d" % big)):
        poses, shifts, counts, g = _run(prediction, forest, model, row, frames, shift)
        assert (g["uniform"], g["px"], g["py"], g["tiles_x"], g["tiles_y"]) == (1, geo.px, geo.py, geo.tiles_x, geo.tiles_y), g
        assert (g["rw"], g["rh"], 1 << g["swz_log2"]) == (geo.rw, geo.rh, geo.m), g
        runs[mode] = (poses, shifts, counts)
        for i in range(n):
            want = cached.predict(forest, model, frames[i], K)
            assert np.array_equal(poses["mid_point"][i], want.mid_point) and np.array_equal(poses["rotation"][i], want.rotation), f"{mode}: frame {i}"
    assert runs["auto"][0].tobytes() == runs["off"][0].tobytes() == runs["forced"][0].tobytes()

    for i, (_, s, _) in enumerate(ref):
        assert tuple(runs["auto"][1][i]) == s, f"frame {i}: shift {tuple(runs['auto'][1][i])}, restatement {s}"
    assert runs["auto"][1].any()
    assert not runs["off"][1].any()
    assert (runs["forced"][1] == big).all()
    assert np.array_equal(runs["auto"][2], tsr.per_list([c for _, _, c in ref]))
    assert np.array_equal(runs["off"][2], tsr.per_list([c for c, _, _ in ref]))
    assert np.array_equal(runs["forced"][2], tsr.per_list([int(m.sum()) for m in maps]))

    # the taps of product mode (guess grids, hit counts, position votes) under each of the three
    tile = {} if row["tile"] is None else {"DH_TILE": "%d,%d" % row["tile"]}
    hits = 0
    for shift in (None, "off", "%d,%d" % big):
        knobs = dict(tile, **row["knobs"])
        if shift:
            knobs["DH_TILE_SHIFT"] = shift
        with env(DH_TILE=None, DH_TILE_SHIFT=None):
            hits += _product_mode_check(prediction, cached, forest, model, frames, K, knobs)
    assert hits > 0


# ================================================================== (b) request kinds
W, H, STEP, PX, PY = 324, 244, 4, 12, 8
TILE = f"{PX},{PY}"
MODEL = synth.ModelParams(stepwidth=STEP)
GEO = tsr.Geometry(W, H, STEP, (80, 80), (24, 24), (PX, PY))
SHIFT_MODES = (("off", "off"), ("auto", None), ("0,0", "0,0"), ("8,7", "8,7"))
RADIUS = 20


@pytest.fixture(scope="module")
def forest():
    return synth.fit_forest(6, 9, synth.FOREST_SEED_BASE + 83, n_frames=10, subset=1500)     # the forest of tests/test_gpu_tile_shift.py


@pytest.fixture(scope="module")
def tables(forest):
    return sr.LeafTables(forest)


def kind_frames():
    """The 19 frames of tests/test_gpu_tile_shift.py (subjects, empty, noise, corner blobs, blobs on tile borders), the last four
    with a second head beside the first."""
    from test_gpu_tile_shift import _frames
    f = _frames()
    other = synth.biwi_batch(4, W, H, first=1100)
    for i in range(4):
        moved = np.zeros_like(other[i])
        s = W // 3
        if i % 2:
            moved[:, s:] = other[i][:, :W - s]
        else:
            moved[:, :W - s] = other[i][:, s:]
        f[15 + i] = hr.composite(f[15 + i], moved)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def frames():
    return kind_frames()


def K0():
    return synth.default_intrinsic(W, H)


def _want_shifts(frs, block=8):
    ref, _ = tsr.choice(frs, GEO, block)
    return [s for _, s, _ in ref], [c for _, _, c in ref]


def _under_every_mode(prediction, forest, n, call, chunk_starts=(0,), frames_for_choice=None):
    """call(hp) -> bytes, on a fresh predictor under each of SHIFT_MODES: the bytes are the same, the shifts are zero / chosen /
    forced as the mode says, and the automatic choice and its list lengths are the restatement's.  Returns the bytes."""
    out = {}
    for mode, shift in SHIFT_MODES:
        with env(DH_TILE=TILE, DH_TILE_SHIFT=shift):
            with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
                raw = call(hp)
                shifts, counts = hp.debug_tile_shifts(n)
        out[mode] = raw
        if mode == "auto":
            assert shifts.any()
            if frames_for_choice is not None:
                want, tiles = _want_shifts(frames_for_choice)
                assert [tuple(s) for s in shifts] == want
                assert np.array_equal(counts, tsr.per_list(tiles, chunk_starts))
        elif mode == "off":
            assert not shifts.any()
        else:
            assert (shifts == tuple(int(v) for v in mode.split(","))).all()
    for mode in out:
        assert out[mode] == out["off"], f"{mode} differs from the fixed grid"
    return out["auto"]


def test_support_records(mods, oracle, cached, forest, tables, frames):
    """predict_batch_support and its device form: poses and support records."""
    import torch
    _lib, prediction, _ = mods
    n = frames.shape[0]
    intr = prediction.IntrinsicMatrix(K0())
    want = np.zeros(n, dtype=_lib.SUPPORT_DTYPE)
    mids = np.zeros((n, 3), np.float32)
    mg, mask = sr.head_guesses(cached, forest, MODEL, frames, K0())      # the mean shift starts on the votes: cubes that hold some
    for i in range(n):
        res, rec, _ = sr.support_ref(cached, tables, MODEL, frames[i], K0(), RADIUS, mg[i] if mask[i] & 1 else None)
        want[i], mids[i] = sr.as_record(rec, _lib.SUPPORT_DTYPE), res.mid_point
    assert sr.partial(want) >= 2, want

    def host(hp):
        poses, sup = hp.predict_batch_support(frames, intr, RADIUS, mg, None, mask)
        return poses.tobytes() + sup.tobytes()

    dev = torch.device("cuda", 0)
    ft = torch.from_numpy(np.array(frames).view(np.int16)).to(dev)
    gmt, gkt = torch.from_numpy(mg).to(dev), torch.from_numpy(mask).to(dev)

    def device(hp):
        out = torch.zeros(n * _lib.POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        sup = torch.zeros(n * _lib.SUPPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        hp.predict_batch_support_device(ft.data_ptr(), n, W, H, intr, out.data_ptr(), sup.data_ptr(), RADIUS, gmt.data_ptr(), None, gkt.data_ptr(),
                                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy().tobytes() + sup.cpu().numpy().tobytes()

    raw = _under_every_mode(prediction, forest, n, host, frames_for_choice=frames)
    assert _under_every_mode(prediction, forest, n, device, frames_for_choice=frames) == raw
    poses = np.frombuffer(raw[:n * _lib.POSE_DTYPE.itemsize], dtype=_lib.POSE_DTYPE)
    sup = np.frombuffer(raw[n * _lib.POSE_DTYPE.itemsize:], dtype=_lib.SUPPORT_DTYPE)
    assert np.array_equal(poses["mid_point"], mids)
    assert sup.tobytes() == want.tobytes(), [(i, sup[i], want[i]) for i in range(n) if sup[i].tobytes() != want[i].tobytes()][:4]


def test_heads(mods, oracle, cached, forest, tables, frames):
    """predict_heads with max_heads 2 on frames four of which hold two heads: head counts and head records (pose and support)."""
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

    raw = _under_every_mode(prediction, forest, n, call, frames_for_choice=frames)
    assert raw == want_n.tobytes() + want.tobytes()


def test_camera_table(mods, oracle, cached, forest, frames):
    """predict_batch_cameras: a matrix per frame, one of them no pinhole."""
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

    poses = np.frombuffer(_under_every_mode(prediction, forest, n, call, frames_for_choice=frames), dtype=_lib.POSE_DTYPE)
    for i in range(n):
        want = cached.predict(forest, MODEL, frames[i], Ks[i])
        assert np.array_equal(poses["mid_point"][i], want.mid_point) and np.array_equal(poses["rotation"][i], want.rotation), f"frame {i}"


def test_guesses_with_a_mask(mods, oracle, cached, forest, frames):
    """Guesses for some frames only (mask bit 0: midpoint, bit 1: rotation)."""
    _lib, prediction, _ = mods
    n = frames.shape[0]
    rs = np.random.RandomState(5)
    mg = np.stack([rs.uniform(-80, 80, n), rs.uniform(-60, 60, n), rs.uniform(700, 1100, n)], 1).astype(np.float32)
    rg = rs.uniform(-1.0, 1.0, (n, 3))
    mask = (np.arange(n) % 4).astype(np.uint8)
    poses = np.frombuffer(_under_every_mode(prediction, forest, n, lambda hp: hp.predict_batch(frames, prediction.IntrinsicMatrix(K0()), mg, rg, mask).tobytes(),
                                            frames_for_choice=frames), dtype=_lib.POSE_DTYPE)
    for i in range(n):
        want = cached.predict(forest, MODEL, frames[i], K0(), mg[i] if mask[i] & 1 else None, rg[i] if mask[i] & 2 else None)
        assert np.array_equal(poses["mid_point"][i], want.mid_point) and np.array_equal(poses["rotation"][i], want.rotation), f"frame {i}"


def _oracle_poses(cached, forest, frs):
    return [cached.predict(forest, MODEL, f, K0()) for f in frs]


def _assert_poses(poses, want, what):
    for i, r in enumerate(want):
        assert np.array_equal(poses["mid_point"][i], r.mid_point) and np.array_equal(poses["rotation"][i], r.rotation), f"{what}: frame {i}"


def _device_call(torch, prediction, _lib, frs, stream):
    """hp -> pose bytes of predict_batch_device on `stream` (frames uploaded once)."""
    dev = torch.device("cuda", 0)
    n = frs.shape[0]
    ft = torch.from_numpy(np.array(frs).view(np.int16)).to(dev)
    torch.cuda.synchronize()

    def call(hp):
        out = torch.zeros(n * _lib.POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        hp.predict_batch_device(ft.data_ptr(), n, W, H, prediction.IntrinsicMatrix(K0()), out.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        return out.cpu().numpy().tobytes()
    return call


def test_device_batch_on_a_side_stream(mods, oracle, cached, forest, frames):
    import torch
    _lib, prediction, _ = mods
    n = frames.shape[0]
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    raw = _under_every_mode(prediction, forest, n, _device_call(torch, prediction, _lib, frames, stream), frames_for_choice=frames)
    _assert_poses(np.frombuffer(raw, dtype=_lib.POSE_DTYPE), _oracle_poses(cached, forest, frames), "side stream")


@pytest.mark.parametrize("chunks,n", [(2, 35), (3, 54)])
def test_forked_sub_batches(mods, oracle, cached, forest, frames, chunks, n):
    """set_forking(2) on 35 frames: sub-batches of 17 and 18, the second from frame 17 (no multiple of 8); set_forking(3) on 54: three of
    18.  Each passes 512 tiles and writes lists of its own; debug_tile_shifts gives the shifts of the whole slice and the summed lengths."""
    import torch
    _lib, prediction, _ = mods
    idx = np.random.RandomState(n).permutation(n) % frames.shape[0]
    frs = np.ascontiguousarray(frames[idx])
    starts = tuple(n * c // chunks for c in range(chunks))
    assert starts[1] % 8 != 0 and all((b - a) * GEO.tiles > 512 for a, b in zip(starts, starts[1:] + (n,)))
    inner = _device_call(torch, prediction, _lib, frs, torch.cuda.current_stream())

    def call(hp):
        hp.set_forking(chunks)
        return inner(hp)

    raw = _under_every_mode(prediction, forest, n, call, chunk_starts=starts, frames_for_choice=frs)
    want = _oracle_poses(cached, forest, frames)
    _assert_poses(np.frombuffer(raw, dtype=_lib.POSE_DTYPE), [want[i] for i in idx], f"{chunks} sub-batches")
    with env(DH_TILE=TILE, DH_TILE_SHIFT=None):
        with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
            assert inner(hp) == raw                        # one kernel sequence: the same bytes


def test_graph_replayed_over_rewritten_frames(mods, oracle, cached, forest, frames):
    """graph_capture once, three launches; between them the frames are rewritten in place: a permutation of the batch, then a batch whose
    frame 0 is empty.  Each launch equals a fresh run without a graph, and its shifts are the restatement's for the frames it saw."""
    import torch
    _lib, prediction, _ = mods
    n = frames.shape[0]
    dev = torch.device("cuda", 0)
    perm = np.random.RandomState(3).permutation(n)
    third = np.ascontiguousarray(frames[perm][::-1]).copy()
    third[0] = 0
    batches = [np.array(frames), np.array(frames[perm]), third]
    for mode, shift in SHIFT_MODES:
        with env(DH_TILE=TILE, DH_TILE_SHIFT=shift):
            with prediction.HoughPrediction(forest, MODEL, device=0) as hp, prediction.HoughPrediction(forest, MODEL, device=0) as fresh:
                buf = torch.from_numpy(batches[0].view(np.int16)).to(dev)
                out = torch.zeros(n * _lib.POSE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                hp.reserve(n, W, H)
                hp.graph_capture(buf.data_ptr(), n, W, H, prediction.IntrinsicMatrix(K0()), out.data_ptr())
                st = torch.cuda.current_stream(dev)
                for k, frs in enumerate(batches):
                    buf.copy_(torch.from_numpy(frs.view(np.int16)))
                    hp.graph_launch(st.cuda_stream)
                    torch.cuda.synchronize()
                    got = out.cpu().numpy().tobytes()
                    assert got == fresh.predict_batch(frs, prediction.IntrinsicMatrix(K0())).tobytes(), f"{mode}: launch {k}"
                    shifts, counts = hp.debug_tile_shifts(n)
                    if mode == "auto":
                        want, tiles = _want_shifts(frs)
                        assert shifts.any() and [tuple(s) for s in shifts] == want, f"launch {k}"
                        assert np.array_equal(counts, tsr.per_list(tiles)), f"launch {k}"
                    if mode == "off":
                        assert not shifts.any()
                    if k == 0:
                        first = got
                    _assert_poses(np.frombuffer(got, dtype=_lib.POSE_DTYPE), _oracle_poses(cached, forest, frs), f"{mode}: launch {k}")
        if mode == "off":
            ref = first
        assert first == ref


# ================================================================== (c) state across batches on one predictor
def _sequence(prediction, forest, batches, **knobs):
    """Pose bytes, shifts and counts (None for a batch that ran without lists) of the batches run in order on ONE predictor."""
    out = []
    with env(DH_TILE=TILE, **knobs):
        with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
            for frs in batches:
                poses = hp.predict_batch(frs, prediction.IntrinsicMatrix(K0()))
                if frs.shape[0] * GEO.tiles > 512:
                    out.append((poses.tobytes(), *hp.debug_tile_shifts(frs.shape[0])))
                else:
                    with pytest.raises(Exception, match="ran without tile lists"):
                        hp.debug_tile_shifts(frs.shape[0])
                    out.append((poses.tobytes(), None, None))
    return out


def test_big_small_big_on_one_predictor(mods, oracle, cached, forest, frames):
    """A batch with lists and shifts, a 3-frame batch (no lists, the fixed grid; debug_tile_shifts says so), then the first batch with its
    frames rolled by 5 slots: each equals a fresh predictor's and the oracle's."""
    _lib, prediction, _ = mods
    batches = [np.ascontiguousarray(frames), np.ascontiguousarray(frames[3:6]), np.ascontiguousarray(np.roll(frames, 5, axis=0))]
    seq = _sequence(prediction, forest, batches, DH_TILE_SHIFT=None)
    for k, frs in enumerate(batches):
        (raw, shifts, counts), = _sequence(prediction, forest, [frs], DH_TILE_SHIFT=None)
        assert seq[k][0] == raw, f"batch {k}"
        _assert_poses(np.frombuffer(raw, dtype=_lib.POSE_DTYPE), _oracle_poses(cached, forest, frs), f"batch {k}")
        if shifts is not None:
            want, tiles = _want_shifts(frs)
            assert seq[k][1].any() and [tuple(s) for s in seq[k][1]] == want == [tuple(s) for s in shifts]
            assert np.array_equal(seq[k][2], tsr.per_list(tiles)) and np.array_equal(counts, seq[k][2])
    assert seq[1][1] is None


def test_content_that_leaves_a_slot_and_comes_back(mods, oracle, cached, forest, frames):
    """Slot 9 holds a blob top-left, then nothing, then a blob bottom-right, over three batches with lists (k_boxsum's sparse stores:
    "zero over zero is not written again" on the masks the shifts are chosen from).  With DH_BOX_DENSE=1 (every cell stored, no masks,
    no shift) the bytes are the same."""
    _lib, prediction, _ = mods
    batches = []
    for k in range(3):
        b = np.array(frames)
        b[9] = 0
        if k == 0:
            b[9, :70, :90] = 900
        if k == 2:
            b[9, H - 70:, W - 90:] = 900
        b[2], b[3] = frames[3 + k], frames[2]          # and ordinary content that moves between slots
        batches.append(b)
    seq = _sequence(prediction, forest, batches, DH_TILE_SHIFT=None)
    dense = _sequence(prediction, forest, batches, DH_TILE_SHIFT=None, DH_BOX_DENSE="1")
    for k, frs in enumerate(batches):
        (raw, shifts, counts), = _sequence(prediction, forest, [frs], DH_TILE_SHIFT=None)
        assert seq[k][0] == raw == dense[k][0], f"batch {k}"
        _assert_poses(np.frombuffer(raw, dtype=_lib.POSE_DTYPE), _oracle_poses(cached, forest, frs), f"batch {k}")
        want, tiles = _want_shifts(frs)
        assert seq[k][1].any() and [tuple(s) for s in seq[k][1]] == want
        assert np.array_equal(seq[k][2], tsr.per_list(tiles))
        assert not dense[k][1].any()
        assert np.array_equal(dense[k][2], tsr.per_list([c for c, _, _ in tsr.choice(frs, GEO, 8)[0]]))


# ================================================================== (d) the LDS limit of k_tile_shift's table
def test_lds_limit_on_the_device(mods, forest):
    """800 x 600 in tiles of 16 x 6 windows (12 x 22 = 264 tiles: two frames reach the lists).  With 8-row mask blocks -- a workspace
    of the two frames -- the occupancy table does not fit k_tile_shift's LDS: the fixed grid, and a forced shift is refused with the
    frame size.  With 16-row blocks -- the smallest workspace that takes them -- it fits: shifts are chosen, the poses stay."""
    _lib, prediction, _ = mods
    w, h, tile = 800, 600, (16, 6)
    geo = tsr.Geometry(w, h, STEP, (80, 80), (24, 24), tile)
    n = 2
    assert n * geo.tiles > 512 and geo.block(n) == 8 and not geo.fits(8) and not geo.fits(8, forced=True)
    cap16 = next(c for c in range(n, 4096) if geo.block(c) == 16)
    assert geo.block(cap16 - 1) == 8 and geo.chooses(16) and geo.forced(4, 1) == (4, 1)
    frs = synth.biwi_batch(n, w, h, first=620)
    intr = prediction.IntrinsicMatrix(synth.default_intrinsic(w, h))

    def run(shift, reserve=0):
        with env(DH_TILE="%d,%d" % tile, DH_TILE_SHIFT=shift):
            with prediction.HoughPrediction(forest, MODEL, device=0) as hp:
                if reserve:
                    hp.reserve(reserve, w, h)
                poses = hp.predict_batch(frs, intr)
                g = hp.debug_geometry()
                assert (g["uniform"], g["px"], g["py"]) == (1,) + tile
                return (poses.tobytes(), *hp.debug_tile_shifts(n))

    off = run("off")
    small = run(None)
    assert small[0] == off[0] and not small[1].any() and np.array_equal(small[2], off[2])
    with pytest.raises(Exception, match="800x600"):
        run("4,1")
    ref, _ = tsr.choice(frs, geo, 16)
    large = run(None, reserve=cap16)
    assert large[0] == off[0] and large[1].any()
    assert [tuple(s) for s in large[1]] == [s for _, s, _ in ref]
    assert np.array_equal(large[2], tsr.per_list([c for _, _, c in ref]))
    forced = run("4,1", reserve=cap16)
    assert forced[0] == off[0] and (forced[1] == (4, 1)).all()
    last = run(None, reserve=cap16 - 1)                  # the capacity just below: 8-row blocks again
    assert last[0] == off[0] and not last[1].any() and np.array_equal(last[2], off[2])
