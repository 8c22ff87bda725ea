"""Per-frame shift of k_traverse's tile grid (k_tile_shift): poses do not depend on it, the choice is the one a numpy restatement
makes on the same occupancy, and the paths without a choice keep the fixed grid.

Geometry: frames of 324 x 244 at stride 4 are 61 x 41 windows; DH_TILE=12,8 cuts them into 6 x 6 tiles with a slack of 11 window
columns and 7 rows, so a frame chooses among sx in {0, 4, 8} and sy in 0 .. 7, and 19 frames have 684 tiles (the tile lists serve
batches of more than 512)."""
import contextlib
import os

import numpy as np
import pytest

import tile_shift_ref as tsr
from depthhead_amd import synth

pytestmark = pytest.mark.gpu

W, H, STEP, PX, PY = 324, 244, 4, 12, 8
TILE = f"{PX},{PY}"


@pytest.fixture(scope="module")
def hp_mod(hip_lib):
    from depthhead_amd import prediction
    return prediction


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def forest():
    return synth.fit_forest(6, 9, synth.FOREST_SEED_BASE + 83, n_frames=10, subset=1500)


MODEL = synth.ModelParams(stepwidth=STEP)
RW = RH = 24                       # the fitted forests' one rectangle size (80 x 0.3)
TBW = (PX - 1) * STEP + 80 - RW + 1      # columns / rows of rectangle sums under a full tile
TBH = (PY - 1) * STEP + 80 - RH + 1


def _frames():
    """19 frames (not a multiple of 8): subjects, empty, noise, a blob in each corner, blobs whose rectangle sums begin or end exactly
    on a tile border of the unshifted grid (columns 48 k, rows 32 k) and of shifted ones (48 k - 4 sx, 32 k - 4 sy)."""
    f = synth.biwi_batch(19, W, H, first=600)
    rs = np.random.RandomState(8)
    f[6] = 0
    f[7] = rs.randint(400, 1400, (H, W)).astype(np.uint16)
    for i, (ys, xs) in enumerate(((slice(0, 70), slice(0, 90)), (slice(0, 70), slice(W - 90, W)),
                                  (slice(H - 70, H), slice(0, 90)), (slice(H - 70, H), slice(W - 90, W)))):
        f[8 + i] = 0
        f[8 + i][ys, xs] = 900
    # the rectangle with origin (x, y) sums pixels [x, x + 24) x [y, y + 24): pixels from column c on make the sums non-zero from c - 23 on
    f[12] = 0; f[12, 32 + 23:150, 48 + 23:200] = 900         # sums begin at column 48 / row 32: the unshifted grid's borders
    f[13] = 0; f[13, 28 + 23:150, 32 + 23:200] = 900         # ... at 32 / 28: the borders under the shift (4, 1)
    f[14] = 0; f[14, 60:96, 100:144] = 900                   # sums end at column 143 / row 95: the last before the borders 144 / 96
    return f


@pytest.fixture(scope="module")
def frames():
    fr = _frames()
    fr.setflags(write=False)
    return fr


def _run(hp_mod, forest, frames, reserve=0, w=W, h=H, second=None, **kv):
    """Poses, shifts and list counts of one batch (and of a second one on the same predictor) under DH_TILE and the given knobs."""
    with env(DH_TILE=TILE, **kv):
        with hp_mod.HoughPrediction(forest, MODEL, device=0) as hp:
            if reserve:
                hp.reserve(reserve, w, h)
            K = hp_mod.IntrinsicMatrix(synth.default_intrinsic(w, h))
            out = []
            for fr in (frames,) if second is None else (frames, second):
                poses = hp.predict_batch(fr, K)
                shifts, counts = hp.debug_tile_shifts(fr.shape[0])
                out.append((poses.tobytes(), poses, shifts, counts))
            geo = hp.debug_geometry()
    assert (geo["uniform"], geo["px"], geo["py"]) == (1, PX, PY) and (geo["rw"], geo["rh"]) == (RW, RH)
    return out[0] if second is None else out


@pytest.fixture(scope="module")
def off(hp_mod, forest, frames):
    return _run(hp_mod, forest, frames, DH_TILE_SHIFT="off")


# ------------------------------------------------------------------ the choice, restated (tests/tile_shift_ref.py, at this geometry)
def _geo(w=W, h=H):
    return tsr.Geometry(w, h, STEP, (80, 80), (RW, RH), (PX, PY))


def _occupancy(frame, block):
    return tsr.occupancy(frame, block, (RW, RH))


def _tiles(occ, sx, sy, tiles_x, tiles_y):
    geo = _geo()
    assert (geo.tiles_x, geo.tiles_y) == (tiles_x, tiles_y)
    return tsr.tiles(occ, geo, sx, sy)


def _choice(frames, block, w=W, h=H):
    return tsr.choice(frames, _geo(w, h), block)


_per_list = tsr.per_list


# ------------------------------------------------------------------ poses
def test_geometry_has_the_slack_the_cases_need(hp_mod, forest, frames, off):
    assert MODEL.patch_grid(W, H) == (61, 41)
    _, shifts = _choice(frames[:0], 8)
    assert len(shifts) == 3 * 8 and shifts[0] == (0, 0) and shifts[-1] == (8, 7)
    assert not off[2].any()


def test_poses_under_the_chosen_shifts(hp_mod, oracle, forest, frames, off):
    """Byte-identical to the fixed grid and exact against the oracle; some frames did choose a shift, and the empty and the
    all-noise frame (every shift ties) keep (0, 0)."""
    raw, poses, shifts, counts = _run(hp_mod, forest, frames)
    assert raw == off[0]
    K = synth.default_intrinsic(W, H)
    for i in range(frames.shape[0]):
        ref = oracle.predict(forest, MODEL, frames[i], K)
        assert np.array_equal(poses["mid_point"][i], ref.mid_point) and np.array_equal(poses["rotation"][i], ref.rotation), f"frame {i}"
    assert shifts.any()
    assert not shifts[6].any() and not shifts[7].any()
    assert counts.sum() <= off[3].sum()


def test_poses_under_every_forced_shift(hp_mod, forest, frames, off):
    """Each allowed DH_TILE_SHIFT=sx,sy, both extremes included: the same bytes, with tiles cut at the left and top edge holding the
    corner blobs' windows.  A shift beyond the slack is clamped to the allowed set; anything else is refused."""
    for sy in range(8):
        for sx in (0, 4, 8):
            raw, _, shifts, counts = _run(hp_mod, forest, frames, DH_TILE_SHIFT=f"{sx},{sy}")
            assert raw == off[0], f"shift {sx},{sy}"
            assert (shifts == (sx, sy)).all(), f"shift {sx},{sy}"
            if (sx, sy) == (0, 0):
                assert np.array_equal(counts, off[3])         # the masks' rule at (0, 0) is the rule of k_boxsum's flags
    raw, _, shifts, _ = _run(hp_mod, forest, frames, DH_TILE_SHIFT="100,100")
    assert raw == off[0] and (shifts == (8, 7)).all()
    _, _, shifts, _ = _run(hp_mod, forest, frames, DH_TILE_SHIFT="6,3")
    assert (shifts == (4, 3)).all()
    for bad in ("on", "4", "-4,0", "4,1,2"):
        with pytest.raises(Exception, match="DH_TILE_SHIFT"):
            _run(hp_mod, forest, frames, DH_TILE_SHIFT=bad)


# ------------------------------------------------------------------ the choice
# k_boxsum's mask blocks are 8 rows high in a workspace of these 19 frames and 32 rows, as on large batches, from 110 frames on
# (reserve picks the shortest of 8, 16, 32 rows whose waves still fit the chip at once).
@pytest.mark.parametrize("reserve,block", [(0, 8), (128, 32)])
def test_choice_against_a_numpy_restatement(hp_mod, forest, frames, off, reserve, block):
    ref, _ = _choice(frames, block)
    _, _, shifts, counts = _run(hp_mod, forest, frames, reserve=reserve)
    for i, (_, s, _) in enumerate(ref):
        assert tuple(shifts[i]) == s, f"frame {i}: shift {tuple(shifts[i])}, restatement {s}"
    assert np.array_equal(counts, _per_list([c for _, _, c in ref]))
    raw0, _, shifts0, counts0 = _run(hp_mod, forest, frames, reserve=reserve, DH_TILE_SHIFT="0,0")
    raw_off, _, _, counts_off = _run(hp_mod, forest, frames, reserve=reserve, DH_TILE_SHIFT="off")
    assert raw0 == off[0] and raw_off == off[0]
    assert np.array_equal(counts0, counts_off) and np.array_equal(counts0, _per_list([c for c, _, _ in ref]))
    assert counts.sum() <= counts_off.sum()
    for i, (c0, _, c) in enumerate(ref):
        assert c <= c0, f"frame {i}"


def test_ordinary_subjects_walk_strictly_fewer_tiles(hp_mod, forest, frames):
    """The ordinary-subject frames of the batch alone (ten of them, twice: 20 x 36 tiles > 512): the lists the GPU wrote hold
    strictly fewer tiles under the chosen shifts than under the fixed grid."""
    ordinary = np.concatenate([frames[:6], frames[15:]] * 2)
    _, _, shifts, counts = _run(hp_mod, forest, ordinary)
    _, _, _, counts_off = _run(hp_mod, forest, ordinary, DH_TILE_SHIFT="off")
    assert shifts.any() and counts.sum() < counts_off.sum()


def test_second_batch_on_the_same_predictor(hp_mod, forest, frames, off):
    """Shifts are per batch: a second batch of other frames (16 ordinary subjects) gets its own, nothing of the first survives, and
    for ordinary subjects the chosen grids have strictly fewer tiles than the fixed one."""
    second = synth.biwi_batch(16, W, H, first=4000)
    (raw_a, _, sh_a, cn_a), (raw_b, _, sh_b, cn_b) = _run(hp_mod, forest, frames, second=second)
    off_a, off_b = _run(hp_mod, forest, frames, second=second, DH_TILE_SHIFT="off")
    assert raw_a == off_a[0] == off[0] and raw_b == off_b[0]
    ref, _ = _choice(second, 8)
    assert [tuple(s) for s in sh_b] == [s for _, s, _ in ref]
    assert np.array_equal(cn_b, _per_list([c for _, _, c in ref]))
    assert np.array_equal(off_b[3], _per_list([c for c, _, _ in ref]))
    assert cn_b.sum() < off_b[3].sum()
    assert not off_b[2].any()


def test_geometry_without_slack_keeps_the_fixed_grid(hp_mod, forest):
    """320 x 240 at stride 4 is 60 x 40 windows, whole tiles of 12 x 8: the one shift (0, 0), the lists of the fixed grid."""
    w, h = 320, 240
    assert MODEL.patch_grid(w, h) == (60, 40)
    fr = synth.biwi_batch(21, w, h, first=900)                  # 21 x 25 tiles > 512
    raw, _, shifts, counts = _run(hp_mod, forest, fr, w=w, h=h)
    raw_off, _, _, counts_off = _run(hp_mod, forest, fr, w=w, h=h, DH_TILE_SHIFT="off")
    assert raw == raw_off and not shifts.any() and np.array_equal(counts, counts_off)
    ref, _ = _choice(fr, 8, w, h)
    assert np.array_equal(counts, _per_list([c for c, _, _ in ref]))
