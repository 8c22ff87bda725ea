"""Numpy restatement of the per-frame shift of k_traverse's tile grid (k_tile_shift) and of the host rules
the choice depends on, for any frame size, stride, patch, rectangle, tile and mask block height.

TEST INFRASTRUCTURE ONLY.  Written from the prose of dh_host.h / DESIGN.md; nothing here is imported from the library.

The rule: k_boxsum leaves, per frame, one bit per group of 4 columns x `block` rows of rectangle origins, set when a rectangle
with its origin in the group has a non-zero sum.  The tile (tx, ty) of the grid shifted by (sx, sy) windows holds the windows
[tx px - sx, (tx + 1) px - sx) x [ty py - sy, (ty + 1) py - sy) (clipped to the frame's windows); its region of rectangle origins
is [X, X + tbw) x [Y, Y + tbh) with X = (tx px - sx) step, tbw = (px - 1) step + patch width - rw + 1 (rows alike), and it is
flagged when that region meets the columns and rows of a set group.  A frame takes the allowed shift with the fewest flagged
tiles, ties to the smallest sy, then the smallest sx.
"""
from __future__ import annotations

import math

import numpy as np

BOX_SPAN = 256                  # image columns one k_boxsum wave spans
LDS_WORDS = 12288               # k_tile_shift's table: 48 KB
WAVE_BUDGET = 12 * 256          # k_boxsum waves the chip holds at once: 12 per CU


# ------------------------------------------------------------------ the host rules
def swizzle_m(step: int) -> int:
    """Planes a row of rectangle sums is de-interleaved into: the largest power of two dividing the stride, at most 8."""
    m = 1
    while m < 8 and step % (2 * m) == 0:
        m *= 2
    return m


def shift_step(step: int) -> int:
    """gx: the steps in windows sx moves in.  A shift of s windows moves a tile's first column by s * step / m words of its plane,
    and that has to stay a whole number of 16-byte pieces (4 words): s * step must be a multiple of 4 m."""
    m4 = 4 * swizzle_m(step)
    return m4 // math.gcd(step, m4)


def patch_grid(w: int, h: int, step: int, sw: int, sh: int) -> tuple[int, int]:
    """Sliding windows of a frame: centres from half a patch in, every `step` pixels, while the patch stays inside."""
    nx = len(range(sw // 2, w - (sw - sw // 2), step)) if w >= sw else 0
    ny = len(range(sh // 2, h - (sh - sh // 2), step)) if h >= sh else 0
    return nx, ny


def box_split(w: int, rw: int) -> tuple[int, int]:
    """(box_parts, box_ow): a k_boxsum wave yields up to (256 - rw) & ~3 of the w - rw + 1 columns of rectangle sums; the parts
    share them evenly, in whole groups of 4."""
    bw, ow_max = w - rw + 1, (BOX_SPAN - rw) & ~3
    parts = -(-bw // ow_max)
    return parts, min(ow_max, (-(-bw // parts) + 3) & ~3)


def block_height(cap: int, parts: int, rows: int) -> int:
    """Rows of a mask block in a workspace of `cap` frames: the first of 8 and 16 whose waves (frames x parts x blocks) fit the
    chip at once, else 32."""
    for blk in (8, 16):
        if cap * parts * -(-rows // blk) <= WAVE_BUDGET:
            return blk
    return 32


def lds_words(mask_blocks: int, parts: int, nc: int, n_shifts: int) -> int:
    """Words of k_tile_shift's LDS: the mask words (two each), the summed-area table over (blocks + 1) x (groups + 1), a counter
    per shift and 8 more."""
    return 2 * mask_blocks * parts + (mask_blocks + 1) * (nc + 1) + n_shifts + 8


class Geometry:
    """Everything the rule needs of one geometry.  patch = (sw, sh), rect = (rw, rh), tile = (px, py) as the tile chooser or
    DH_TILE gave it (at most the frame's windows)."""

    def __init__(self, w, h, step, patch=(80, 80), rect=(24, 24), tile=(12, 8)):
        self.w, self.h, self.step = int(w), int(h), int(step)
        self.sw, self.sh = patch
        self.rw, self.rh = rect
        self.nx, self.ny = patch_grid(self.w, self.h, self.step, self.sw, self.sh)
        self.px, self.py = min(tile[0], self.nx), min(tile[1], self.ny)
        self.tiles_x, self.tiles_y = -(-self.nx // self.px), -(-self.ny // self.py)
        self.tiles = self.tiles_x * self.tiles_y
        self.slack_x, self.slack_y = self.tiles_x * self.px - self.nx, self.tiles_y * self.py - self.ny
        self.m, self.gx = swizzle_m(self.step), shift_step(self.step)
        self.tbw = (self.px - 1) * self.step + self.sw - self.rw + 1        # columns / rows of rectangle sums under a full tile
        self.tbh = (self.py - 1) * self.step + self.sh - self.rh + 1
        self.box_rows = self.h - self.rh + 1
        self.box_parts, self.box_ow = box_split(self.w, self.rw)

    def shifts(self):
        """The allowed shifts, in the order ties are broken in: sy-major."""
        return [(sx, sy) for sy in range(self.slack_y + 1) for sx in range(0, self.slack_x + 1, self.gx)]

    def forced(self, sx: int, sy: int) -> tuple[int, int]:
        """A forced shift as it runs: clamped to the slack, sx rounded down to a multiple of gx."""
        return min(sx, self.slack_x) // self.gx * self.gx, min(sy, self.slack_y)

    def largest_shift(self) -> tuple[int, int]:
        return self.forced(1 << 20, 1 << 20)

    def block(self, cap: int) -> int:
        return block_height(cap, self.box_parts, self.box_rows)

    def lds(self, block: int, forced: bool = False) -> int:
        n_shifts = 1 if forced else len(self.shifts())
        return lds_words(-(-self.box_rows // block), self.box_parts, self.box_parts * (self.box_ow // 4), n_shifts)

    def fits(self, block: int, forced: bool = False) -> bool:
        return self.lds(block, forced) <= LDS_WORDS

    def chooses(self, block: int) -> bool:
        """Do frames of this geometry choose a shift (automatic path)?  Some slack, and the table fits."""
        return len(self.shifts()) > 1 and self.fits(block)


# ------------------------------------------------------------------ the choice
def occupancy(frame, block: int, rect=(24, 24)):
    """Pixel-resolution image of k_boxsum's masks: True over the 4 columns x `block` rows of every group that holds a rectangle
    origin with a non-zero sum.  (Origins right of w - rw are left out: their clipped rectangles lie inside that of column w - rw,
    and no tile's region holds one of them without it.)"""
    rw, rh = rect
    h, w = frame.shape
    sat = np.zeros((h + 1, w + 1), np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(frame > 0, axis=0), axis=1)
    nz = (sat[rh:, rw:] - sat[:-rh, rw:] - sat[rh:, :-rw] + sat[:-rh, :-rw]) > 0       # [h - rh + 1][w - rw + 1]
    rows, cols = nz.shape
    occ = np.zeros((-(-rows // block) * block, -(-cols // 4) * 4), bool)
    occ[:rows, :cols] = nz
    g = occ.reshape(occ.shape[0] // block, block, occ.shape[1] // 4, 4).any(axis=(1, 3))
    return np.repeat(np.repeat(g, block, axis=0), 4, axis=1)


def flag_map(occ, geo: Geometry, sx: int, sy: int):
    """[tiles_y][tiles_x] bool: tiles of the grid shifted by (sx, sy) windows whose region of rectangle origins meets the occupancy."""
    out = np.zeros((geo.tiles_y, geo.tiles_x), bool)
    for ty in range(geo.tiles_y):
        for tx in range(geo.tiles_x):
            x, y = (tx * geo.px - sx) * geo.step, (ty * geo.py - sy) * geo.step
            out[ty, tx] = occ[max(y, 0):max(y + geo.tbh, 0), max(x, 0):max(x + geo.tbw, 0)].any()
    return out


def tiles(occ, geo: Geometry, sx: int, sy: int) -> int:
    """Tiles of the grid shifted by (sx, sy) windows whose region of rectangle origins meets the occupancy."""
    return int(flag_map(occ, geo, sx, sy).sum())


def choice(frames, geo: Geometry, block: int):
    """Per frame: tiles at shift (0, 0), the chosen shift (fewest tiles, ties to the smallest (sy, sx)) and its tiles; and the
    allowed shifts."""
    shifts = geo.shifts()
    res = []
    for fr in frames:
        occ = occupancy(fr, block, (geo.rw, geo.rh))
        counts = [tiles(occ, geo, sx, sy) for sx, sy in shifts]
        best = min(range(len(shifts)), key=lambda i: (counts[i], shifts[i][1], shifts[i][0]))
        res.append((counts[0], shifts[best], counts[best]))
    return res, shifts


def forced_counts(frames, geo: Geometry, block: int, sx: int, sy: int):
    """Per frame: the flag map under one shift for every frame."""
    return [flag_map(occupancy(fr, block, (geo.rw, geo.rh)), geo, sx, sy) for fr in frames]


def per_list(per_frame, starts=(0,)):
    """Tiles per list: a frame goes to the list of its index within its kernel sequence mod 8.  `starts` are the first frames of
    the sequences (forked sub-batches each count from their own first frame; their lists are summed)."""
    out = np.zeros(8, np.int64)
    for i, c in enumerate(per_frame):
        out[(i - max(s for s in starts if s <= i)) % 8] += c
    return out
