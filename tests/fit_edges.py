"""Placed rows for the fit family's point correspondence (DH_FIT_CORRESPOND, depthhead_amd/csrc/dh_fit_device.h; DESIGN.md section
18a): one-point models that sit ON a compare of the chain, or one representable step to either side of it, with the answer of each
row -- `points` (0 or 1) and `sum_r2_fixed` -- written down as literals worked by hand.  No restatement produced them;
test_fit_edges_ref.py holds the five restatements to them and test_gpu_fit_edges.py every entry point of the GPU.

THE GEOMETRY.  Frame 16 x 12, K = [[16, 0, 8], [0, 16, 6], [0, 0, 1]], R = I, scale = 1, t = (0, 0, 64).  A point v is posed to
p = v + t, and with the normal nm = (0, 0, -1)
    c = -p.z,   x = (16 p.x + 8 p.z) / p.z,   y = (16 p.y + 6 p.z) / p.z,   res = c * (d / p.z - 1).
Every row keeps p.z a power of two (64, 1, 16, 512, 65536) wherever a value has to be exact, so each product is a shift, each sum
has a handful of bits and the quotients divide by a power of two: the values are the same in f32 and f64 and no rounding happens.
At p.z = 64:  x = p.x / 4 + 8,  y = p.y / 4 + 6,  c = -64,  res = -(d - 64), so a kept row whose pixel holds 64 + g adds
g * g * 2^20 to sum_r2_fixed.  At p.z = 1: x = 16 p.x + 8, c = -1, res = -(d - 1).  At p.z = 512: x = p.x / 32 + 8, c = -512 and
d = 256 gives res = -512 * (1/2 - 1) = 256.  At p.z = 65536: d = 65535 gives d / p.z - 1 = -2^-16 and res = 1.
Where p.z is NOT a power of two (a row one step off in z) the row is a dropped one, so its residual is never formed; its pixel is
aimed at the middle of a pixel, where the rounding of x and y cannot change (int)x, (int)y.
The steps are the f32 spacing of the coordinate that moves: 2^-18 at 32 and 63, 2^-19 at 24 and just below 32, 2^-20 at 14 and
in 2^-20 itself, 2^-15 at 448.

THE RULE THAT MAKES A ROW TIGHT.  A dropped row fails exactly ONE link (`link`); every other link would pass for it, and the pixel
that the relaxed compare would read holds a depth inside the gate.  So relaxing that one compare -- in a kernel, in one expansion
or in one restatement -- keeps the row and changes the record.  The frames are BACK = 69 (64 + 5, inside both gates at p.z = 64)
wherever no row says otherwise; a wrongly kept row at p.z = 64 therefore shows as one more point and 25 * 2^20 more.  For y == h
and for the corner row the relaxed read lies outside the frame: in the next frame (BACK again), or, for the last frame, in the
guard band that the _device tests put around the frames.

Kept rows carry distinct g (2, 4, 8, 16, 1 and the gates' +-25 / +-256), so in the aggregated form sum_r2_fixed tells which rows
were kept.  The gate rows exist once per gate: a row with `gate` set belongs only to the table of that gate (the fit's 25 and 256,
the shape family's largest)."""
import collections

import numpy as np

W, H = 16, 12
K = np.array([[16, 0, 8], [0, 16, 6], [0, 0, 1]], np.float32)
T = (0.0, 0.0, 64.0)
BACK = 69
GATES = (25.0, 256.0)
GRAZE = 0.9216                      # min_cos2 of the grazing rows: (24 / 25)^2, the f64 nearest to it
LINKS = ("pz", "c", "x_lo", "x_hi", "y_lo", "y_hi", "pixel", "gate", "graze")
INST_DTYPE = np.dtype([("frame", "<u4"), ("mesh", "<u4"), ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"), ("flags", "<u4")],
                      align=True)      # dh_render_instance
assert INST_DTYPE.itemsize == 64

Row = collections.namedtuple("Row", "name v nm pix reads points e link gate K t graze last")


def _row(name, v, pix, points, e, link=None, nm=(0, 0, -1), reads=None, gate=None, K=None, t=None, graze=None, last=False):
    """pix: ((px, py), depth) pairs the row needs; reads: the pixel the row -- or the compare relaxed -- reads, None when it lies
    outside the frame (default: the first of pix); graze: `points` under the surface step's grazing test at GRAZE where that
    differs from `points`."""
    assert (points == 0) == (link is not None) and (points == 1 or e == 0) and (link is None or link in LINKS)
    if reads is None and pix:
        reads = pix[0][0]
    return Row(name, tuple(float(np.float32(c)) for c in v), tuple(float(c) for c in nm), tuple(pix), reads, points, e, link, gate,
               None if K is None else np.array(K, np.float32).reshape(3, 3), None if t is None else tuple(float(c) for c in t),
               points if graze is None else graze, last)


M20 = 1 << 20
_K_NEG_Z = [[16, 0, 0], [0, 16, 0], [0, 0, -1]]

ROWS = (
    # ---- p.z >= 1.0.  p.z = 1: x = 16 * 2.5/16 + 8 = 10.5, y = 6.5; c = -1; d = 3: res = -(3 - 1) = -2, e = 4 * 2^20.
    _row("pz_on", (2.5 / 16, 0.5 / 16, -63.0), [((10, 6), 3)], 1, 4 * M20),
    # p.z = 1 - 2^-18 (63 + 2^-18 is an f32).  x = 3.5 / p.z + 8 = 11.50001..; the pixel holds 2, |2 - p.z| < 25.
    _row("pz_below", (3.5 / 16, 0.5 / 16, -63.0 - 2.0 ** -18), [((11, 6), 2)], 0, 0, "pz"),
    # ---- the pixel.  d = 1 at p.z = 1: gap 0, res = -1 * (1 / 1 - 1) = 0: kept with e = 0 (a pixel of 1 is a depth, not a hole).
    _row("pixel_one", (4.5 / 16, 0.5 / 16, -63.0), [((12, 6), 1)], 1, 0),
    # d = 0 at p.z = 16 (x = p.x + 8 = 6.5, y = 6.5): |0 - 16| = 16 is inside both gates, so only `pixel != 0` drops it.
    _row("pixel_zero", (-1.5, 0.5, -48.0), [((6, 6), 0)], 0, 0, "pixel"),
    # ---- c < 0.0.  nm = (-1, 0, 0), p = (2^-10, -10, 64): c = -2^-10 (tiny, negative): kept.  x = 8 + 2^-12, y = 3.5; d = 80:
    # res = -2^-10 * (80 / 64 - 1) = -2^-12, res^2 * 2^20 = 2^-4, which truncates to 0.
    _row("c_tiny", (2.0 ** -10, -10.0, 0.0), [((8, 3), 80)], 1, 0, nm=(-1, 0, 0)),
    # nm = (1, 0, 0), p = (0, 4, 64): c = (1 * 0 + 0 * 4) + 0 * 64 = 0 exactly.  x = 8, y = 7: the pixel is BACK.
    _row("c_zero", (0.0, 4.0, 0.0), [], 0, 0, "c", nm=(1, 0, 0), reads=(8, 7)),
    # ---- x's low edge.  p.x = -32: x = (-512 + 512) / 64 = 0, y = -18 / 4 + 6 = 1.5; d = 68: e = 4^2 * 2^20.
    _row("x_zero", (-32.0, -18.0, 0.0), [((0, 1), 68)], 1, 16 * M20),
    # p.x = -32 - 2^-18: x = -2^-14 / 64 = -2^-20; (int)x = 0, so x >= 0 relaxed reads pixel (0, 2) = BACK.
    _row("x_below_zero", (-32.0 - 2.0 ** -18, -14.0, 0.0), [], 0, 0, "x_lo", reads=(0, 2)),
    # ---- x's high edge.  p.x = 32 - 2^-19: x = 16 - 2^-21, (int)x = 15; y = 3.5; d = 72: e = 8^2 * 2^20.
    _row("x_below_w", (32.0 - 2.0 ** -19, -10.0, 0.0), [((15, 3), 72)], 1, 64 * M20),
    # p.x = 32: x = 16 = w, y = 4.5: x < w relaxed reads frame[4 * 16 + 16], the first pixel of the next row, (0, 5) = BACK.
    _row("x_equals_w", (32.0, -6.0, 0.0), [], 0, 0, "x_hi", reads=(0, 5)),
    # ---- y, the same four.  p.y = -24: y = 0, x = 2.5; d = 80: e = 16^2 * 2^20.
    _row("y_zero", (-22.0, -24.0, 0.0), [((2, 0), 80)], 1, 256 * M20),
    # p.y = -24 - 2^-19: y = -2^-21: relaxed reads (3, 0) = BACK.
    _row("y_below_zero", (-18.0, -24.0 - 2.0 ** -19, 0.0), [], 0, 0, "y_lo", reads=(3, 0)),
    # p.y = 24 - 2^-19: y = 12 - 2^-21, (int)y = 11; x = 4.5; d = 65: e = 1 * 2^20.
    _row("y_below_h", (-14.0, 24.0 - 2.0 ** -19, 0.0), [((4, 11), 65)], 1, 1 * M20),
    # p.y = 24: y = 12 = h, x = 5.5: y < h relaxed reads a whole row past the frame, frame[12 * 16 + 5].
    _row("y_equals_h", (-10.0, 24.0, 0.0), [], 0, 0, "y_hi", reads=None),
    # ---- the gate, at 25.  p.z = 64, d = 89 and 39: gap = +25 and -25 = the gate: kept, e = 25^2 * 2^20 = 655360000 each.
    _row("gate25_above_on", (-26.0, 10.0, 0.0), [((1, 8), 89)], 1, 625 * M20, gate=25.0),
    _row("gate25_below_on", (-22.0, 10.0, 0.0), [((2, 8), 39)], 1, 625 * M20, gate=25.0),
    # one step beyond: p.z = 64 - 2^-20 under d = 89 (gap 25 + 2^-20), p.z = 64 + 2^-20 over d = 39 (gap -25 - 2^-20).
    _row("gate25_above_beyond", (-18.0, 10.0, -2.0 ** -20), [((3, 8), 89)], 0, 0, "gate", gate=25.0),
    _row("gate25_below_beyond", (-14.0, 10.0, 2.0 ** -20), [((4, 8), 39)], 0, 0, "gate", gate=25.0),
    # ---- the gate, at 256.  d = 320 at p.z = 64: gap = +256, res = -256, e = 2^16 * 2^20.  d = 256 at p.z = 512 (x = p.x / 32 + 8
    # = 2.5, y = 80 / 32 + 6 = 8.5): gap = -256, c = -512, res = -512 * (256 / 512 - 1) = 256, e = 2^16 * 2^20.
    _row("gate256_above_on", (-26.0, 10.0, 0.0), [((1, 8), 320)], 1, 65536 * M20, gate=256.0),
    _row("gate256_below_on", (-176.0, 80.0, 448.0), [((2, 8), 256)], 1, 65536 * M20, gate=256.0),
    # one step beyond: p.z = 64 - 2^-20 under d = 320; p.z = 512 + 2^-15 over d = 256 (x = 4.4999.., y = 8.4999..).
    _row("gate256_above_beyond", (-18.0, 10.0, -2.0 ** -20), [((3, 8), 320)], 0, 0, "gate", gate=256.0),
    _row("gate256_below_beyond", (-112.0, 80.0, 448.0 + 2.0 ** -15), [((4, 8), 256)], 0, 0, "gate", gate=256.0),
    # ---- the surface step's grazing test, c * c >= min_cos2 * |p|^2, at min_cos2 = GRAZE.  p = (0, 14, 48): c = -48, c^2 = 2304,
    # |p|^2 = (0 + 196) + 2304 = 2500 and GRAZE * 2500 rounds to 2304 exactly (asserted in test_fit_edges_ref.py): kept.  x = 384 /
    # 48 = 8, y = 512 / 48 = 10.67; d = 48 = p.z: res = -48 * (48 / 48 - 1) = 0.  p.y one step (2^-20) smaller: |p|^2 smaller, kept;
    # one step larger: dropped by the grazing test alone.  Everywhere but in the surface step all three are kept.
    _row("graze_on", (0.0, 14.0, -16.0), [((8, 10), 48)], 1, 0),
    _row("graze_inside", (0.0, 14.0 - 2.0 ** -20, -16.0), [((8, 10), 48)], 1, 0),
    _row("graze_outside", (0.0, 14.0 + 2.0 ** -20, -16.0), [((8, 10), 48)], 1, 0, graze=0),
    # ---- the corner: x = 16 on row 11 (y = 11.5) of the LAST frame: x < w relaxed reads frame[11 * 16 + 16], one element past it.
    _row("corner", (32.0, 22.0, 0.0), [], 0, 0, "x_hi", reads=None, last=True),
    # ---- rows with a pose or a K of their own (the per-row form through a camera table only).
    # x = -0.0: K = [[16, 0, 0], [0, 16, 0], [0, 0, -1]] at p = (0, 0, 64): r0 = (0 * 16 + 0 * 0) + 64 * 0 = 0, r2 = -64, x = y = 0 / -64
    # = -0.0, and -0.0 >= 0.0: kept at pixel (0, 0); d = 66: e = 2^2 * 2^20.
    _row("x_negative_zero", (0.0, 0.0, 0.0), [((0, 0), 66)], 1, 4 * M20, K=_K_NEG_Z),
    # d = 65535, the largest pixel, at p.z = 65536 (t.z = 65536): gap = -1, d / p.z - 1 = -2^-16, res = -65536 * -2^-16 = 1.
    _row("pixel_65535", (0.0, 0.0, 0.0), [((8, 6), 65535)], 1, 1 * M20, t=(0, 0, 65536)),
    # a third row of zeros: r2 = 0; r0 = 512 > 0, r1 = 384 > 0: x = y = +inf.
    _row("k_inf", (0.0, 0.0, 0.0), [], 0, 0, "x_hi", reads=None, K=[[16, 0, 8], [0, 16, 6], [0, 0, 0]]),
    # K = 0: x = y = 0 / 0 = NaN, which fails every compare of the frame test.
    _row("k_nan", (0.0, 0.0, 0.0), [], 0, 0, "x_lo", reads=None, K=np.zeros((3, 3))),
    # r2 = -64 at p = (0, -40, 64): x = 512 / -64 = -8, y = (-640 + 384) / -64 = 4: only x >= 0 fails; relaxed it reads frame[4 * 16 - 8].
    _row("k_negative_r2", (0.0, -40.0, 0.0), [], 0, 0, "x_lo", reads=(8, 3), K=[[16, 0, 8], [0, 16, 6], [0, 0, -1]]),
)
GRAZING = ("graze_on", "graze_inside", "graze_outside")
FILLER = ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))        # p = (0, 0, 64), c = +64: always culled at c < 0
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


def rows_of(gate, own=True):
    """The rows of the table of `gate`; own=False: only those that use the table's K and t.  A `last` row comes last."""
    rows = [r for r in ROWS if r.gate in (None, float(gate)) and (own or (r.K is None and r.t is None))]
    return sorted(rows, key=lambda r: r.last)


def frame_of(rows, back=BACK):
    """A 12 x 16 frame of `back` with the pixels of `rows`; two rows may share a pixel only with the same depth."""
    f = np.full((H, W), back, np.uint16)
    seen = {}
    for r in rows:
        for (px, py), d in r.pix:
            assert seen.setdefault((px, py), d) == d, (r.name, px, py)
            f[py, px] = d
    return f


def model_of(rows, mirrored=False):
    """(points [n, 3] f32, normals [n, 3] f32); mirrored: v -> -2 v for scale = -1/2 (the products v * scale are the same, exactly)."""
    pts = np.array([r.v if isinstance(r, Row) else r[0] for r in rows], np.float32).reshape(-1, 3)
    nrm = np.array([r.nm if isinstance(r, Row) else r[1] for r in rows], np.float32).reshape(-1, 3)
    return (pts * np.float32(-2.0) if mirrored else pts), nrm


def instance(frame, model, t=T, mirrored=False, flags=0):
    out = np.zeros((), INST_DTYPE)
    out["frame"], out["mesh"], out["R"], out["t"], out["scale"], out["flags"] = frame, model, np.eye(3, dtype=np.float32).reshape(9), t, \
        (-0.5 if mirrored else 1.0), flags
    return out


Table = collections.namedtuple("Table", "rows frames Ks models inst points e index")


def per_row(gate, mirrored=False, own=True):
    """One one-point model, one frame (with its K) and one instance per row, so that record i names row i."""
    rows = rows_of(gate, own)
    frames = np.stack([frame_of([r]) for r in rows])
    Ks = np.stack([K if r.K is None else r.K for r in rows]).astype(np.float32)
    models = [model_of([r], mirrored) for r in rows]
    inst = np.array([instance(i, i, T if r.t is None else r.t, mirrored, 0x5A0000 + i) for i, r in enumerate(rows)], INST_DTYPE)
    return Table(rows, frames, Ks, models, inst, [r.points for r in rows], [r.e for r in rows], {r.name: i for i, r in enumerate(rows)})


def slots(n):
    """The model indices that the rows of an aggregated model of n points take, in the order they are handed out: 0, 63, 64, 255
    and 256 (and 1023, 1024 where n allows) first -- the first and last lane of a wave, the last lane of the workgroup, the first
    point of the second stride, either side of the LDS staging budget -- then their neighbours, outwards."""
    anchors = [(0, 1), (63, -1), (64, 1), (255, -1), (256, 1), (1023, -1), (1024, 1)]
    out = []
    for k in range(n):
        for a, d in anchors:
            i = a + k * d
            if 0 <= i < n and i not in out:
                out.append(i)
    return out


def aggregated(n, gate, mirrored=False, pin=None, only=None, graze=False):
    """All rows that use the table's K and t in ONE model of n points and one frame, at the indices of slots(n) among filler points
    (nm = (0, 0, +1): culled at c).  pin = (name, index) puts that row at that index; only: the names of the rows to take (default
    all).  points and e are the sums of the literals (graze=True: of the surface step at GRAZE, which is meant for
    only=GRAZING -- at GRAZE the rows away from the optical axis fail the grazing test too)."""
    rows = [r for r in rows_of(gate, own=False) if only is None or r.name in only]
    free = slots(n)
    index = {}
    if pin is not None:
        index[pin[0]] = pin[1]
        free.remove(pin[1])
    for r in rows:
        if r.name not in index:
            index[r.name] = free.pop(0)
    items = [FILLER] * n
    for r in rows:
        items[index[r.name]] = r
    inst = np.array([instance(0, 0, T, mirrored, 0x5A0000)], INST_DTYPE)
    kept = [r for r in rows if (r.graze if graze else r.points)]
    return Table(rows, frame_of(rows)[None], K[None].copy(), [model_of(items, mirrored)], inst, len(kept), sum(r.e for r in kept), index)


def lone_frame(row):
    """A frame of zeros but for the pixel that `row` (or its relaxed compare) reads: a second view that sees this row alone."""
    f = np.zeros((H, W), np.uint16)
    if row.reads is not None:
        f[row.reads[1], row.reads[0]] = dict(row.pix).get(row.reads, BACK)
    return f


# ---- the aggregated model as a triangle mesh, for the entry points that take a subject set (its normals come from the mesh)
Mesh = collections.namedtuple("Mesh", "verts tris table")
FAR = 1000.0


def aggregated_mesh(n, gate, mirrored=False, only=None):
    """aggregated(n, gate, ...) with triangles that give every point the table's normal EXACTLY: each row is one corner of a
    triangle of its own, which lies in the plane through the row's point across its normal and has legs of FAR along two axes,
    so that two components of the face product are sums of products with 0 and the third over its own magnitude is +-1.  The
    two other corners of a row's triangle take filler indices; they carry the row's normal and are dropped well away from any
    compare: FAR along x or y they project a hundred pixels outside the frame, FAR along z they face a depth far beyond the
    gate or have c = 0.  Every other filler is a corner of a triangle with two shared vertices in the plane z = 0, wound to
    nm = (0, 0, +1).  The Table's model holds the mesh's vertices and the normals the set must arrive at."""
    tb = aggregated(n, gate, mirrored, only=only)
    pts, nrm = tb.models[0]
    verts, want = pts.astype(np.float32).copy(), nrm.copy()
    spare = [i for i in range(n) if i not in tb.index.values()][::-1]       # from the far end, away from the rows
    flip = np.float32(-2.0 if mirrored else 1.0)
    tris = []
    legs = {(0.0, 0.0, -1.0): ((0, FAR, 0), (FAR, 0, 0)), (-1.0, 0.0, 0.0): ((0, 0, FAR), (0, FAR, 0)), (1.0, 0.0, 0.0): ((0, FAR, 0), (0, 0, FAR))}
    for r in tb.rows:
        a = tb.index[r.name]
        b, c = spare.pop(), spare.pop()
        for j, leg in ((b, legs[r.nm][0]), (c, legs[r.nm][1])):
            verts[j] = (np.float32(r.v) + np.float32(leg)) * flip
            want[j] = r.nm
        tris.append((a, b, c))
    h1, h2 = spare.pop(), spare.pop()
    verts[h1], verts[h2] = np.float32((FAR, 0, 0)) * flip, np.float32((0, FAR, 0)) * flip
    tris += [(i, h1, h2) for i in spare]
    model = (verts, want)
    return Mesh(verts, np.array(tris, np.uint32), tb._replace(models=[model]))


def as_dicts(inst):
    """The instances as the dicts that the set restatements take (frame, R [3, 3], t, scale)."""
    return [{"frame": int(i["frame"]), "R": i["R"].reshape(3, 3).copy(), "t": i["t"].copy(), "scale": float(i["scale"])} for i in inst]


def tracker_inputs(n_cameras=1):
    """What puts the table's exact start into a fit tracker: a pose with rotation (0, 0, 0) -- entry 60 of the
    angle table, cos = 1 and sin = 0, so R = X (Y Z) is the identity but for signed zeros -- and mid_point = T, with a support
    that counts as a detection; and tracker parameters under which the fit is accepted as it stands (no step when carried, no
    point, rms or jump limit in reach), so that the next step starts from the very same R and t, carried.
    -> (poses, support, tracker parameters as keywords)."""
    poses = np.zeros(n_cameras, np.dtype([("mid_point", "<f4", (3,)), ("reserved", "<u4"), ("rotation", "<f8", (3,))], align=True))
    poses["mid_point"] = T
    support = np.zeros(n_cameras, np.dtype([("x", "<u4"), ("y", "<u4"), ("width", "<u4"), ("height", "<u4"), ("windows", "<u4"),
                                            ("hits", "<u4"), ("mass", "<u8"), ("total_mass", "<u8")], align=True))
    support["windows"], support["hits"], support["mass"], support["total_mass"] = 1, 1, 1, 1
    return poses, support, dict(iterations_tracked=0, keep_points=0, rms_max=4096.0, max_jump=4096.0)
