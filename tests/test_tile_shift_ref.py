"""tests/tile_shift_ref.py against definitions that do not share its code: the flagged tiles are conservative for every allowed
shift (brute force from the pixels), at shift (0, 0) they are the tiles k_boxsum's flag rule marks, and the host rules (gx, mask
block height, LDS fit) give the values worked out by hand from dh_host.h."""
import numpy as np
import pytest

import tile_shift_ref as tsr

# (w, h, stride, patch, rectangle, tile, mask block height): strides 1, 4, 6 and 16, a rectangle that is not square, widths with
# w % 4 != 0, every block height; each has at least two sx and two sy to choose from
GEOMETRIES = [
    (101, 97, 1, (80, 80), (24, 24), (13, 6), 8),
    (230, 170, 4, (100, 80), (30, 18), (10, 8), 16),
    (262, 200, 6, (80, 80), (21, 21), (12, 8), 32),
    (420, 300, 16, (80, 80), (24, 24), (5, 4), 8),
    (163, 131, 4, (80, 80), (32, 32), (5, 4), 16),
]


def _sparse_frames(w, h, seed):
    """Seeded sparse frames: a few lone pixels, a small blob, pixels in the corners and on the last row / column, and an empty one."""
    rs = np.random.RandomState(seed)
    out = np.zeros((5, h, w), np.uint16)
    for k in range(6):
        out[0, rs.randint(h), rs.randint(w)] = 1 + rs.randint(3000)
    y, x = rs.randint(h - 20), rs.randint(w - 30)
    out[1, y:y + 1 + rs.randint(20), x:x + 1 + rs.randint(30)] = 900
    out[2, 0, 0] = out[2, h - 1, w - 1] = out[2, 0, w - 1] = out[2, h - 1, 0] = 7
    out[3, rs.randint(h), w - 1] = 5
    out[3, h - 1, rs.randint(w)] = 5
    return out


def _windows_with_content(frame, geo):
    """[ny][nx] bool, by brute force: the window's patch [i step, i step + sw) x [j step, j step + sh) holds a non-zero pixel."""
    hit = np.zeros((geo.ny, geo.nx), bool)
    for y, x in zip(*np.nonzero(frame)):
        for j in range(geo.ny):
            if not (j * geo.step <= y < j * geo.step + geo.sh):
                continue
            for i in range(geo.nx):
                if i * geo.step <= x < i * geo.step + geo.sw:
                    hit[j, i] = True
    return hit


@pytest.mark.parametrize("w,h,step,patch,rect,tile,block", GEOMETRIES)
def test_flagged_tiles_hold_every_window_with_content(w, h, step, patch, rect, tile, block):
    geo = tsr.Geometry(w, h, step, patch, rect, tile)
    shifts = geo.shifts()
    assert len({sx for sx, _ in shifts}) >= 2 and len({sy for _, sy in shifts}) >= 2
    assert shifts[0] == (0, 0) and shifts[-1] == geo.largest_shift()
    seen = 0
    for k, fr in enumerate(_sparse_frames(w, h, 11 + step)):
        hit = _windows_with_content(fr, geo)
        assert fr.any() or not hit.any()
        seen += int(hit.sum())
        occ = tsr.occupancy(fr, block, rect)
        for sx, sy in shifts:
            fm = tsr.flag_map(occ, geo, sx, sy)
            for j, i in zip(*np.nonzero(hit)):
                assert fm[(j + sy) // geo.py, (i + sx) // geo.px], f"frame {k}, shift {sx},{sy}: window {i},{j} in an unflagged tile"
            assert tsr.tiles(occ, geo, sx, sy) == fm.sum()
    assert seen > 0


def _groups(frame, geo, block):
    """Set groups (block row b, column group c) by brute force: a pixel (y, x) makes the sums of the origins
    [x - rw + 1, x] x [y - rh + 1, y] non-zero; the origins run to w - rw and h - rh."""
    out = set()
    for y, x in zip(*np.nonzero(frame)):
        for oy in range(max(y - geo.rh + 1, 0), min(y, geo.h - geo.rh) + 1):
            for ox in range(max(x - geo.rw + 1, 0), min(x, geo.w - geo.rw) + 1):
                out.add((oy // block, ox // 4))
    return out


@pytest.mark.parametrize("w,h,step,patch,rect,tile,block", GEOMETRIES)
def test_shift_zero_is_the_rule_of_the_flags(w, h, step, patch, rect, tile, block):
    """k_boxsum's flags: tile (tx, ty) is marked when [tx tpx, tx tpx + tbw) x [ty tpy, ty tpy + tbh) meets a set group."""
    geo = tsr.Geometry(w, h, step, patch, rect, tile)
    tpx, tpy = geo.px * step, geo.py * step
    tbw = (geo.px - 1) * step + patch[0] - rect[0] + 1
    tbh = (geo.py - 1) * step + patch[1] - rect[1] + 1
    for fr in _sparse_frames(w, h, 3 + step):
        groups = _groups(fr, geo, block)
        want = np.zeros((geo.tiles_y, geo.tiles_x), bool)
        for ty in range(geo.tiles_y):
            for tx in range(geo.tiles_x):
                want[ty, tx] = any(4 * c < tx * tpx + tbw and 4 * c + 4 > tx * tpx and b * block < ty * tpy + tbh and (b + 1) * block > ty * tpy
                                   for b, c in groups)
        assert np.array_equal(tsr.flag_map(tsr.occupancy(fr, block, rect), geo, 0, 0), want)


def test_gx_table():
    want = {s: 4 for s in range(1, 13)}
    want.update({16: 2, 24: 4, 32: 1})
    assert {s: tsr.shift_step(s) for s in want} == want
    assert [tsr.swizzle_m(s) for s in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)] == [1, 2, 1, 4, 2, 8, 4, 8, 8, 8]


def test_slack_shifts_and_forced_clamp():
    geo = tsr.Geometry(324, 244, 4)
    assert (geo.nx, geo.ny, geo.tiles_x, geo.tiles_y, geo.slack_x, geo.slack_y) == (61, 41, 6, 6, 11, 7)
    assert geo.shifts() == [(sx, sy) for sy in range(8) for sx in (0, 4, 8)]
    assert geo.forced(100, 100) == (8, 7) and geo.forced(6, 3) == (4, 3) and geo.forced(0, 0) == (0, 0) and geo.forced(11, 7) == (8, 7)
    assert tsr.Geometry(320, 240, 4).shifts() == [(0, 0)]
    g16 = tsr.Geometry(420, 300, 16, tile=(5, 4))
    assert g16.slack_x == 3 and g16.forced(3, 9) == (2, 2)


def test_box_split():
    assert tsr.box_split(324, 24) == (2, 152) and tsr.box_split(255, 24) == (1, 232) and tsr.box_split(256, 24) == (2, 120)
    assert tsr.box_split(520, 24) == (3, 168) and tsr.box_split(800, 24) == (4, 196) and tsr.box_split(322, 21) == (2, 152)


def test_block_height_thresholds():
    """324 x 244 with 24 x 24 rectangles: 2 parts, 221 rows -- 28 blocks of 8 rows, 14 of 16: 8 rows up to 3072 / 56 = 54 frames,
    16 up to 3072 / 28 = 109."""
    geo = tsr.Geometry(324, 244, 4)
    assert (geo.box_parts, geo.box_rows) == (2, 221)
    assert [geo.block(c) for c in (1, 54, 55, 109, 110, 512)] == [8, 8, 16, 16, 32, 32]


def test_lds_fit_on_either_side_of_the_limit():
    """800 x 600, 24 x 24 rectangles: 4 parts of 49 groups, 577 rows.  8-row blocks: 73 blocks, 2 * 73 * 4 + 74 * 197 + shifts + 8
    words, past the 12 288; 16-row blocks: 37 blocks, 296 + 38 * 197 + shifts + 8, inside."""
    geo = tsr.Geometry(800, 600, 4, tile=(16, 6))
    assert (geo.box_parts, geo.box_ow, geo.box_rows, len(geo.shifts())) == (4, 196, 577, 12)
    assert geo.lds(8) == 584 + 14578 + 12 + 8 and geo.lds(16) == 296 + 7486 + 12 + 8 and geo.lds(8, forced=True) == 584 + 14578 + 1 + 8
    assert not geo.fits(8) and not geo.fits(8, forced=True) and geo.fits(16) and not geo.chooses(8) and geo.chooses(16)
    assert geo.block(10) == 8 and geo.block(11) == 16 and geo.block(20) == 16 and geo.block(21) == 32
    # the limit itself: 2 b p + (b + 1)(nc + 1) + s + 8 <= 12288
    assert tsr.lds_words(60, 1, 200, 11) == 120 + 61 * 201 + 19 == 12400
    assert tsr.lds_words(60, 1, 198, 18) == 120 + 61 * 199 + 26 == 12285
    assert tsr.lds_words(60, 1, 198, 21) == tsr.LDS_WORDS and tsr.lds_words(60, 1, 198, 22) == tsr.LDS_WORDS + 1


def test_per_list():
    assert tsr.per_list(range(10)).tolist() == [0 + 8, 1 + 9, 2, 3, 4, 5, 6, 7]
    assert tsr.per_list([1] * 35, starts=(0, 17)).tolist() == [3 + 3, 2 + 3, 2 + 2, 2 + 2, 2 + 2, 2 + 2, 2 + 2, 2 + 2]
