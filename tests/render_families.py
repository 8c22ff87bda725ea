"""Edge families of the renderer: inputs placed on the values at which the rule or the kernels of
k_render.hip change path -- a pixel centre exactly on an edge, a tile seam, the 9-pixel candidate rectangle, the 257th record of
a tile, a depth at a clamp, a snapped coordinate on the guard band, a frame of one pixel.  No GPU import: test_render_families.py
holds tests/render_ref.py to a second statement of the rule on these inputs and test_gpu_render_edges.py holds the GPU to
render_ref.py on them.

A family is a list of cases; a case is a dict: meshes [(verts, tris)], instances (render_ref.instance dicts), n, w, h, K (one
matrix or a per-frame stack), sensor (keyword arguments of render_ref.resolve, {} for none) and reach(census): assertions that
the edge the case is named after is really present, so that a case cannot turn benign without a test failing.

Snapped coordinates are placed exactly: with K = the identity (unit focal length, centre 0) a vertex (sx/16 * z, sy/16 * z, z)
projects to x = sx/16 up to one rounding of the product and one of the quotient, far inside the half unit the snap
floor(16 x + 0.5) forgives; Soup.mesh() asserts through render_ref.transform / project that every vertex snaps to the chosen
integers and keeps the chosen f32 depth.  Coordinates below are in snapped units (1/16 pixel); the centre of pixel column c is
16 c + 8."""
import collections
import functools

import numpy as np

import render_ref as rr

F32 = np.float32
# the screen tile, the per-lane / per-wave threshold and the workgroup of the resolve kernel
DH_RT_W, DH_RT_H, SMALL_PIXELS, LANES, WAVE = 64, 16, 8, 256, 64
KUNIT = np.eye(3, dtype=F32)
EYE = np.eye(3, dtype=F32)
MIRROR = np.diag([-1.0, 1.0, -1.0]).astype(F32)          # a half turn about y: with scale -1 it mirrors y and keeps x and z
INF = float("inf")


def centre(c):
    return 16 * c + 8


def shift(dx_px, dy_px):
    """R that moves an instance by whole pixels on the screen under KUNIT: p0 = v0 + dx * v2, so x = x0 + dx."""
    R = EYE.copy()
    R[0, 2], R[1, 2] = dx_px, dy_px
    return R


def assert_snapped(verts, want, K=KUNIT, R=EYE, t=(0, 0, 0), scale=1.0):
    """The one check every placed mesh passes through: (sx, sy, z) of `want` is what the rule's vertex stage gives."""
    p = rr.transform(verts, np.asarray(R, F32), np.asarray(t, F32), scale)
    fx, fy = rr.project(K, p)
    want = np.asarray(want, dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(fx.astype(np.float64), want[:, 0]) and np.array_equal(fy.astype(np.float64), want[:, 1]), "snapped coordinates moved"
    assert np.array_equal(p[:, 2].astype(np.float64), want[:, 2]), "depths moved"


class Soup:
    """A mesh built from chosen snapped coordinates and f32 depths, three vertices of its own per triangle."""

    def __init__(self):
        self.pts, self.tris = [], []

    def tri(self, a, b, c, z):
        """Triangle a b c (snapped (x, y) pairs); z: one depth or one per vertex."""
        zs = (z, z, z) if np.isscalar(z) else z
        k = len(self.pts)
        for (x, y), zz in zip((a, b, c), zs):
            assert float(F32(zz)) == float(zz), "the depth is no f32"
            self.pts.append((int(x), int(y), float(zz)))
        self.tris.append((k, k + 1, k + 2))
        return self

    def quad(self, x0, y0, x1, y1, z, flip=False):
        """Axis-aligned quad split along the diagonal (x0, y0) - (x1, y1); z at the corners (x0 y0, x1 y0, x1 y1, x0 y1)."""
        zs = (z,) * 4 if np.isscalar(z) else z
        a, b, c, d = (x0, y0), (x1, y0), (x1, y1), (x0, y1)
        if flip:
            self.tri(a, c, b, (zs[0], zs[2], zs[1])).tri(a, d, c, (zs[0], zs[3], zs[2]))
        else:
            self.tri(a, b, c, (zs[0], zs[1], zs[2])).tri(a, c, d, (zs[0], zs[2], zs[3]))
        return self

    def corner(self, c0, r0, bw, bh, z, br=False):
        """A right triangle whose pixel rectangle is exactly columns c0 .. c0 + bw - 1, rows r0 .. r0 + bh - 1: the right angle
        top-left (or bottom-right), the bounding box 2/16 inside the first pixel and 15/16 inside the last."""
        xl, xh, yl, yh = 16 * c0 + 2, 16 * (c0 + bw - 1) + 15, 16 * r0 + 2, 16 * (r0 + bh - 1) + 15
        return self.tri((xh, yh), (xl, yh), (xh, yl), z) if br else self.tri((xl, yl), (xh, yl), (xl, yh), z)

    def mesh(self, cy=0):
        """(verts, tris); cy: the mesh is meant for a K with K[1][2] = cy (pixels), its y is stored relative to that row."""
        pts = np.asarray(self.pts, dtype=np.float64).reshape(-1, 3)
        verts = np.stack([pts[:, 0] / 16.0 * pts[:, 2], (pts[:, 1] - 16.0 * cy) / 16.0 * pts[:, 2], pts[:, 2]], axis=1).astype(F32)
        assert_snapped(verts, pts, K=k_centre(cy))
        return verts, np.asarray(self.tris, dtype=np.uint32).reshape(-1, 3)


def k_centre(cy):
    K = KUNIT.copy()
    K[1, 2] = cy
    return K


def case(label, meshes, instances, n, w, h, reach, K=KUNIT, sensor=None, scene=None):
    """scene: the label of the case whose geometry this one shares (its own by default): the key image is computed once."""
    return {"label": label, "scene": scene or label, "meshes": meshes, "instances": instances, "n": n, "w": w, "h": h, "K": np.asarray(K, F32),
            "sensor": dict(sensor or {}), "reach": reach}


# ------------------------------------------------------------------ the census
def census(c):
    """What the kernels partition a case on, restated from DESIGN.md section 17 in plain Python: the accepted records with the
    tiles each touches and its clipped candidate rectangle (bw, bh) there, records per tile, the number of tiles, the on-edge
    pixel centres (owned: covered with some edge function 0; not_owned: in the pixel rectangle with some edge function 0 and not
    covered), how many records cover each pixel, why triangles were dropped, and the depths at the clamps."""
    n, w, h = c["n"], c["w"], c["h"]
    tiles_x, tiles_y = -(-w // DH_RT_W), -(-h // DH_RT_H)
    K = c["K"]
    Ks = np.broadcast_to(K.reshape(-1, 3, 3), (n, 3, 3)) if K.size == 9 else K.reshape(n, 3, 3)
    records, dropped = [], collections.Counter()
    tile_count = np.zeros((n, tiles_y, tiles_x), dtype=np.int64)
    cover = np.zeros((n, h, w), dtype=np.int32)
    owned, not_owned = set(), set()
    for ii, ins in enumerate(c["instances"]):
        verts, tris = c["meshes"][ins["mesh"]]
        with np.errstate(all="ignore"):                      # (inf * 0 and inf - inf are part of some families)
            p = rr.transform(verts, ins["R"], ins["t"], ins["scale"])
        fx, fy = rr.project(Ks[ins["frame"]], p)
        for ti, tri in enumerate(np.asarray(tris, dtype=np.int64).reshape(-1, 3)):
            z = [float(p[v, 2]) for v in tri]
            sx, sy = [float(fx[v]) for v in tri], [float(fy[v]) for v in tri]
            if any(not (zz >= 1.0) for zz in z):
                dropped["z"] += 1
                continue
            if any(not np.isfinite(v) for v in sx + sy):
                dropped["nonfinite"] += 1
                continue
            if any(abs(v) > rr.GUARD for v in sx + sy):
                dropped["guard"] += 1
                continue
            x, y = [int(v) for v in sx], [int(v) for v in sy]
            area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
            if area == 0:
                dropped["area"] += 1
                continue
            sgn = 1 if area > 0 else -1
            xa, xb = max(-((8 - min(x)) // 16), 0), min((max(x) - 8) // 16, w - 1)
            ya, yb = max(-((8 - min(y)) // 16), 0), min((max(y) - 8) // 16, h - 1)
            if xa > xb or ya > yb:
                dropped["nopixel"] += 1
                continue
            tiles = {}
            for ty in range(ya // DH_RT_H, yb // DH_RT_H + 1):
                for tx in range(xa // DH_RT_W, xb // DH_RT_W + 1):
                    bw = min(xb, tx * DH_RT_W + DH_RT_W - 1) - max(xa, tx * DH_RT_W) + 1
                    bh = min(yb, ty * DH_RT_H + DH_RT_H - 1) - max(ya, ty * DH_RT_H) + 1
                    tiles[(tx, ty)] = (bw, bh)
                    tile_count[ins["frame"], ty, tx] += 1
            # the on-edge centres and the coverage of the pixel rectangle
            py, px = np.meshgrid(np.arange(ya, yb + 1, dtype=np.int64) * 16 + 8, np.arange(xa, xb + 1, dtype=np.int64) * 16 + 8, indexing="ij")
            inside, on_edge = np.ones(px.shape, bool), np.zeros(px.shape, bool)
            for a, b in ((1, 2), (2, 0), (0, 1)):
                dx, dy = sgn * (x[b] - x[a]), sgn * (y[b] - y[a])
                e = dx * (py - y[a]) - dy * (px - x[a])
                inside &= (e >= 0) if (dy < 0 or (dy == 0 and dx > 0)) else (e > 0)
                on_edge |= e == 0
            cover[ins["frame"], ya:yb + 1, xa:xb + 1] += inside
            for r, q in np.argwhere(on_edge):
                (owned if inside[r, q] else not_owned).add((ins["frame"], xa + int(q), ya + int(r), len(records)))
            records.append({"instance": ii, "triangle": ti, "frame": ins["frame"], "x": x, "y": y, "z": z, "head": bool(ins["flags"] & rr.HEAD),
                            "rect": (xa, xb, ya, yb), "tiles": tiles, "covered": int(inside.sum()), "swapped": area < 0})
    keys = expected_keys(c)
    d = np.where(keys != rr.EMPTY, keys >> np.uint32(1), 0)
    return {"records": records, "dropped": dropped, "tile_count": tile_count, "n_tiles": n * tiles_x * tiles_y, "cover": cover,
            "owned": owned, "not_owned": not_owned, "at_1": int((d == 1).sum()), "at_65535": int((d == 65535).sum()), "depth": d,
            "mask": (keys != rr.EMPTY) & ((keys & np.uint32(1)) == 0)}


_KEYS = {}


def expected_keys(c):
    """The restatement's key image of a case: computed once per scene, shared, read-only."""
    if c["scene"] not in _KEYS:
        with np.errstate(all="ignore"):
            keys = rr.render_keys(c["meshes"], c["instances"], c["n"], c["w"], c["h"], c["K"])
        keys.setflags(write=False)
        _KEYS[c["scene"]] = keys
    return _KEYS[c["scene"]]


def expected(c):
    """(frames, masks) of the restatement, sensor model included."""
    return rr.resolve(expected_keys(c), **c["sensor"])


# ------------------------------------------------------------------ centres_on_edges
FAN_RIM = [(64, 0), (64, 32), (48, 48), (32, 64), (0, 64), (-32, 64), (-48, 48), (-64, 32), (-64, 0), (-48, -48), (0, -64), (48, -48)]


def _fan(s, ax, ay, z):
    """Twelve triangles about the apex (ax, ay), every second one wound the other way; the depth falls from the apex outward."""
    for k in range(12):
        a, b = FAN_RIM[k], FAN_RIM[(k + 1) % 12]
        pa, pb = (ax + a[0], ay + a[1]), (ax + b[0], ay + b[1])
        if k % 2:
            s.tri((ax, ay), pb, pa, (z, z + 96.0, z + 64.0))
        else:
            s.tri((ax, ay), pa, pb, (z, z + 64.0, z + 96.0))


def centres_on_edges():
    """Frame 0: a quad whose four edges run through pixel centres, a quad whose diagonal does, a twelve-triangle fan with its apex
    on a centre.  Frames 1 and 2: the same with the owned (left, top) edges
    of one quad and the not owned (right, bottom) edges of another on the centres of column 64 and row 16, the first of the
    next tile, the diagonal across the seam and the fan's apex on that centre.  Frame 3 (principal point in row 20): one quad mesh drawn as it is
    and again at scale -1 under a half turn about y, which mirrors it about that row and turns its winding round."""
    w, h = 96, 40
    zq = (900.0, 964.0, 1028.0, 932.0)
    main = Soup()
    main.quad(centre(2), centre(1), centre(6), centre(5), zq)                       # edges through the centres of columns 2, 6 and rows 1, 5
    main.quad(132, 36, 196, 100, zq, flip=True)                                     # y = x - 96: through (136, 40), (152, 56), ...
    _fan(main, centre(20), centre(10), 700.0)
    both = Soup().quad(centre(30), centre(1), centre(34), centre(5), zq)
    up = [(x, 640 - y, z) for x, y, z in both.pts]
    assert_snapped(both.mesh(cy=20)[0], up, K=k_centre(20), R=MIRROR, scale=-1.0)
    seam = Soup()
    seam.quad(centre(64), centre(16), centre(68), centre(20), zq)                   # owns column 64 and row 16
    seam.quad(centre(60), centre(12), centre(64), centre(16), zq, flip=True)        # ends on them and does not own them
    seam.quad(996, 36, 1060, 100, zq)                                               # y = x - 960 across x = 1024
    fan = Soup()
    _fan(fan, centre(64), centre(16), 700.0)
    meshes = [main.mesh(), both.mesh(cy=20), seam.mesh(), fan.mesh()]
    inst = [rr.instance(0, 0), rr.instance(3, 1), rr.instance(3, 1, MIRROR, scale=-1.0, head=False), rr.instance(1, 2), rr.instance(2, 3, head=False)]
    # centres on the shared edges: the two diagonals and the spokes of both fans
    shared = [(0, c, c - 1) for c in range(3, 6)] + [(0, (136 + 16 * k) // 16, (40 + 16 * k) // 16) for k in range(4)]
    shared += [(3, c, r) for c, r in zip(range(31, 34), range(2, 5))] + [(3, c, 39 - r) for c, r in zip(range(31, 34), range(2, 5))]
    shared += [(1, c, r) for c, r in zip(range(65, 68), range(17, 20))] + [(1, c, r) for c, r in zip(range(61, 64), range(13, 16))]
    shared += [(1, (1000 + 16 * k) // 16, (40 + 16 * k) // 16) for k in range(4)]
    for f, ac, ar in ((0, 20, 10), (2, 64, 16)):
        shared += [(f, ac, ar)] + [(f, ac + k * dx, ar + k * dy) for k in range(1, 4) for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1))]
        shared += [(f, ac + k * dx, ar + k * dy) for k in range(1, 3) for dx, dy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]

    def reach(cs):
        assert len(cs["owned"]) >= 20 and len(cs["not_owned"]) >= 20, (len(cs["owned"]), len(cs["not_owned"]))
        assert cs["cover"].max() == 1                                   # the shapes are disjoint: no pixel twice
        for f, x, y in shared:
            assert cs["cover"][f, y, x] == 1, ("a centre on a shared edge", f, x, y, cs["cover"][f, y, x])
            assert sum(1 for o in cs["owned"] if o[:3] == (f, x, y)) == 1, (f, x, y)
        assert any(f >= 1 and x == 64 for f, x, y, _ in cs["owned"]) and any(f >= 1 and y == 16 for f, x, y, _ in cs["owned"])
        assert any(f == 1 and x == 64 for f, x, y, _ in cs["not_owned"]) and any(f == 1 and y == 16 for f, x, y, _ in cs["not_owned"])
        assert any(r["swapped"] for r in cs["records"]) and not all(r["swapped"] for r in cs["records"])
        assert not any(r["swapped"] for r in cs["records"] if r["instance"] == 1) and all(r["swapped"] for r in cs["records"] if r["instance"] == 2)
        assert not cs["dropped"]

    return [case("centres_on_edges", meshes, inst, 4, w, h, reach, K=np.stack([KUNIT, KUNIT, KUNIT, k_centre(20)]))]


# ------------------------------------------------------------------ tile_seams
SEAM_X = (1015, 1016, 1017, 1031, 1032, 1033)           # 1016 and 1032: the centres of columns 63 and 64; 1/16 either side
SEAM_Y = (247, 248, 249, 263, 264, 265)                 # 248 and 264: the centres of rows 15 and 16


def tile_seams():
    """160 x 40: three tiles each way.  Triangles whose bounding box ends, and others whose box begins, at each of SEAM_X and
    SEAM_Y; two slivers across a seam that cover no centre; one triangle over all nine tiles."""
    w, h = 160, 40
    s = Soup()
    z = 500.0
    for i, v in enumerate(SEAM_X):
        y0 = 20 + 36 * i
        s.tri((v - 50, y0), (v, y0), (v - 50, y0 + 50), z + i)                      # the box ends at x = v
        s.tri((v, y0 + 300), (v + 50, y0 + 300), (v, y0 + 350), z + 10 + i)          # the box begins at x = v
    for i, v in enumerate(SEAM_Y):
        x0 = 20 + 90 * i
        s.tri((x0, v - 50), (x0 + 50, v), (x0, v), z + 20 + i)                      # ends at y = v
        s.tri((x0 + 1300, v), (x0 + 1350, v), (x0 + 1300, v + 50), z + 30 + i)       # begins at y = v
    n_plain = len(s.tris)
    s.tri((1000, 90), (1060, 140), (1062, 140), z + 40)                             # slivers: a box over the seam, no centre inside
    s.tri((700, 240), (760, 270), (760, 272), z + 41)
    s.tri((8, 8), (2500, 8), (8, 630), (800.0, 1200.0, 1000.0))                     # all nine tiles
    meshes = [s.mesh()]

    def reach(cs):
        rec = cs["records"]
        assert len(rec) == n_plain + 3 and not cs["dropped"]
        for axis in (0, 1):
            sides = {tuple(sorted({t[axis] for t in r["tiles"]})) for r in rec[:n_plain]}
            assert {(0,), (1,), (0, 1)} <= sides, (axis, sides)
        assert all(r["covered"] == 0 and len(r["tiles"]) >= 2 for r in rec[n_plain:n_plain + 2])
        assert len(rec[-1]["tiles"]) == 9 and cs["n_tiles"] == 9
        ends = {r["rect"][1] for r in rec[:n_plain]} | {r["rect"][0] for r in rec[:n_plain]}
        assert {62, 63, 64, 65} <= ends

    return [case("tile_seams", meshes, [rr.instance(0, 0)], 1, w, h, reach)]


# ------------------------------------------------------------------ small_big_split
SMALL_RECTS = [(1, 1), (1, 8), (8, 1), (2, 4), (4, 2)]
BIG_RECTS = [(3, 3), (9, 1), (1, 9), (64, 1), (1, 16), (64, 16)]


def small_big_split():
    """128 x 16, two tiles.  In tile 0: the named rectangles, one big record of every width 1 .. 64 at the full height (64 to
    1024 candidates: every row and column div_small can be asked for), right angles top-left and bottom-right in turn so that
    both halves of a rectangle get covered.  One record of columns 63 .. 72: 1 x 4 (small) in tile 0, 9 x 4 (big) in tile 1.  Every
    record has a constant depth of its own, heads and others in turn."""
    w, h = 128, 16
    s = Soup()
    k = 0
    for bw, bh in SMALL_RECTS + BIG_RECTS + [(b, 16) for b in range(1, 65)]:
        s.corner((k * 7) % (64 - bw + 1), (k * 3) % (16 - bh + 1), bw, bh, 1000.0 + 2 * k, br=k % 2 == 1)
        k += 1
    s.corner(63, 5, 10, 4, 990.0)
    heads, others = Soup(), Soup()
    for i, t in enumerate(s.tris):
        (heads if i % 2 == 0 else others).tri(*[s.pts[v][:2] for v in t], s.pts[t[0]][2])
    meshes = [heads.mesh(), others.mesh()]

    def reach(cs):
        rects = [r["tiles"].get((0, 0)) for r in cs["records"]]
        for want in SMALL_RECTS + BIG_RECTS + [(b, 16) for b in range(1, 65)]:
            assert want in rects, want
        both = [r for r in cs["records"] if len(r["tiles"]) == 2]
        assert len(both) == 1 and both[0]["tiles"] == {(0, 0): (1, 4), (1, 0): (9, 4)}
        small = sum(1 for r in rects if r and r[0] * r[1] <= SMALL_PIXELS)
        assert small >= 6 and cs["tile_count"][0, 0, 0] - small >= 64 and cs["tile_count"][0, 0, 0] > WAVE
        assert {8, 9} <= {r[0] * r[1] for r in rects if r} and max(r[0] * r[1] for r in rects if r) == 1024
        assert cs["cover"].max() >= 8 and len(np.unique(cs["depth"])) > 30          # overlapping, and many records win somewhere

    return [case("small_big_split", meshes, [rr.instance(0, 0), rr.instance(0, 1, head=False)], 1, w, h, reach)]


# ------------------------------------------------------------------ deep_lists
DEEP_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


def _tile_soup(count, z0, tile=(0, 0), soup=None, start=0):
    """`count` triangles of 2 x 2 and 3 x 3 pixels inside screen tile `tile`, depth z0 + i."""
    s = Soup() if soup is None else soup
    for i in range(start, start + count):
        size = 2 + i % 2
        s.corner(tile[0] * DH_RT_W + (i * 5) % (DH_RT_W - size + 1), tile[1] * DH_RT_H + (i * 3) % (DH_RT_H - size + 1), size, size,
                 z0 + i, br=i % 4 >= 2)
    return s


def deep_lists():
    """192 x 48, nine tiles holding 0, 1, 63, 64, 65, 255, 256, 257 and 1091 records, from meshes of 1, 2, 255, 256, 257 and 513
    triangles in one call (the setup grid is sized by the largest).  The 513 fill the tiles of 63, 64 and 65 and put 321 into the
    deep one; the meshes of 255, 256 and 257 are drawn into tiles of their own and once more, at scale 2 (twice the depth, the
    same pixels), into the deep one."""
    w, h = 192, 48
    one = Soup().corner(3, 4, 3, 3, (1000.0, 1010.0, 1020.0))
    quad = Soup().quad(centre(10), centre(2), centre(40), centre(12), (1500.0, 1600.0, 1700.0, 1550.0))
    m513 = _tile_soup(63, 5000.0, (2, 0))
    _tile_soup(64, 5000.0, (0, 1), m513, 63)
    _tile_soup(65, 5000.0, (1, 1), m513, 127)
    _tile_soup(321, 5000.0, (2, 2), m513, 192)
    parts = {255: _tile_soup(255, 2000.0), 256: _tile_soup(256, 3000.0), 257: _tile_soup(257, 4000.0)}
    home = {255: (2, 1), 256: (0, 2), 257: (1, 2)}
    for k, s in parts.items():                    # the shifted and the scaled placements snap where they are meant to
        for tile, scale in ((home[k], 1.0), ((2, 2), 2.0)):
            want = [(x + 16 * DH_RT_W * tile[0], y + 16 * DH_RT_H * tile[1], z * scale) for x, y, z in s.pts]
            assert_snapped(s.mesh()[0], want, R=shift(DH_RT_W * tile[0], DH_RT_H * tile[1]), scale=scale)
    meshes = [one.mesh(), quad.mesh(), parts[255].mesh(), parts[256].mesh(), parts[257].mesh(), m513.mesh()]
    assert [len(m[1]) for m in meshes] == [1, 2, 255, 256, 257, 513]
    inst = [rr.instance(0, 5, head=False), rr.instance(0, 0, shift(64, 0)), rr.instance(0, 1, shift(128, 32))]
    for j, k in enumerate((255, 256, 257)):
        inst.append(rr.instance(0, 2 + j, shift(DH_RT_W * home[k][0], DH_RT_H * home[k][1]), head=j % 2 == 0))
        inst.append(rr.instance(0, 2 + j, shift(128, 32), scale=2.0, head=j % 2 == 1))

    def reach(cs):
        counts = sorted(cs["tile_count"].ravel().tolist())
        assert counts[:8] == list(DEEP_COUNTS) and 1024 < counts[8] < 1200, counts
        assert not cs["dropped"] and all(len(r["tiles"]) == 1 for r in cs["records"])
        assert cs["cover"].max() >= 8

    return [case("deep_lists", meshes, inst, 1, w, h, reach)]


# ------------------------------------------------------------------ depth_range
Z_HUGE = float(F32(1.75 * 2.0 ** 127))                  # 2.98e38, the "3e38" of the family
Z_FAR = float(F32(1e30))                               # the f32 next to 1e30
Z_BELOW_ONE = float(np.nextafter(F32(1.0), F32(0.0)))
CONST_DEPTHS = (1.0, Z_BELOW_ONE, 1.25, 2.0, 65534.0, 65534.25, 65535.0, 65536.0, 1e6, Z_HUGE)


def depth_range():
    """48 x 28 under KUNIT (K[0][2] = K[1][2] = 0).  One triangle of constant depth per entry of CONST_DEPTHS (the one just below
    1.0 is dropped; the huge one sits at the origin, where its vertices stay finite); triangles from z = 1 to z = 1e30; a head at
    1e6 and another object at 65536 on the same pixels, both clamped to 65535: the head wins.  A vertex made infinite by the
    scale, and an instance sent to infinite depth by t: their products with the zeros of K and R are NaN, so the rule drops them
    (no vertex of infinite depth survives the projection, whatever K is; 1.0 / z is never 0).  Then the same frame with noise of
    amplitude 3 and of 65535."""
    w, h = 48, 28
    const = Soup()
    for i, z in enumerate(CONST_DEPTHS[:-1]):
        const.corner(2 + 4 * i, 1, 3, 3, z)
    const.tri((0, 0), (18, 0), (0, 18), Z_HUGE)
    slope = Soup()
    # (16 pixels wide: the depth at distance j from the far edge is 16 / j, and 16 / j + 1/2 is no integer for j = 1 .. 16)
    slope.tri((centre(2), centre(6)), (centre(18), centre(6)), (centre(2), centre(14)), (1.0, Z_FAR, 1.0))
    slope.tri((centre(18), centre(6)), (centre(18), centre(14)), (centre(2), centre(14)), (Z_FAR, Z_FAR, 1.0))
    slope.tri((centre(22), centre(6)), (centre(30), centre(6)), (centre(22), centre(14)), (60000.0, 70000.0, 65000.0))
    slope.tri((centre(2), centre(17)), (centre(30), centre(17)), (centre(2), centre(26)), (30000.0, Z_FAR, 40000.0))
    tie_head = Soup().corner(34, 6, 6, 6, 1e6)
    tie_other = Soup().corner(34, 6, 6, 6, 65536.0)
    far = Soup().tri((160, 0), (0, 160), (0, 0), (2.0 ** 100, 2.0 ** 100, 2.0 ** 127))          # at scale 2 the last vertex overflows
    near = Soup().corner(40, 1, 3, 3, 100.0)
    meshes = [const.mesh(), slope.mesh(), tie_head.mesh(), tie_other.mesh(), far.mesh(), near.mesh()]
    inst = [rr.instance(0, 0), rr.instance(0, 1, head=False), rr.instance(0, 3, head=False), rr.instance(0, 2),
            rr.instance(0, 4, scale=2.0), rr.instance(0, 5, t=(0, 0, INF))]

    def reach(cs):
        assert cs["dropped"] == {"z": 1, "nonfinite": 2}, cs["dropped"]
        got = set(np.unique(cs["depth"]).tolist())
        assert {0, 1, 2, 65534, 65535} <= got and cs["at_1"] >= 4 and cs["at_65535"] >= 20, sorted(got)[:8]
        assert cs["depth"][0, 7, 35] == 65535 and cs["mask"][0, 7, 35]              # the tie at the clamp goes to the head
        assert cs["depth"][0, 0, 0] == 65535                                        # the triangle at 2.98e38
        assert len(np.unique(cs["depth"][0, 6:15, 2:21])) > 5 and cs["depth"][0, 6:15, 2:21].max() < 100       # 1 .. 1e30: perspective keeps it near
        far = cs["depth"][0, 17:27, 2:31]
        assert far.max() == 65535 and 30000 <= far[far > 0].min() < 40000 and len(np.unique(far)) > 50          # 30000 .. 1e30 crosses the clamp

    def noisy(a):
        def reach_noise(cs):
            reach(cs)
            clean, _ = rr.resolve(expected_keys(out[0]))
            f, _ = rr.resolve(expected_keys(out[0]), noise=a, seed=5 + a)
            fg = clean > 0
            assert ((f == 1) & fg & (clean > 1)).any() and ((f == 65535) & fg & (clean < 65535)).any()      # clamped at both ends
            assert (f[fg] > 0).all()
        return reach_noise

    out = [case("depth_range", meshes, inst, 1, w, h, reach)]
    for a in (3, 65535):
        out.append(case("depth_range-noise%d" % a, meshes, inst, 1, w, h, noisy(a), sensor={"noise": a, "holes": 0.0, "seed": 5 + a},
                        scene="depth_range"))
    return out


# ------------------------------------------------------------------ guard_band
BAND = 1 << 20


def guard_band():
    """32 x 16.  Frame 0: a triangle with every snapped coordinate at +-2^20 that covers the frame (drawn, 43-bit edge values), its
    twin with one coordinate at 2^20 + 1, nearer (dropped); a small near triangle drawn again and again with NaN, +inf and -inf
    in t, in R and in the scale, with a vertex that the scale carries to +inf, to -inf and (through R) to inf - inf, with scale 0
    and with scale -1 (all dropped).  dh_mesh_create refuses a vertex that is not finite,
    so the vertex gets there through the scale.  Frame 1 has a K with K[2][0] = 1: every vertex of its triangle has p.z >= 1 and
    r2 = p.x + p.z = -64; the rule keeps it."""
    w, h = 32, 16
    big = Soup().tri((BAND, BAND), (-BAND, BAND), (BAND, -BAND), 1024.0)
    twin = Soup().tri((BAND + 1, BAND), (-BAND, BAND), (BAND, -BAND), 512.0)
    near = Soup().corner(4, 3, 5, 5, 100.0)
    edge = (np.array([[3e38, 0, 10], [0, 3e38, 10], [0, 0, 10]], F32), np.array([[0, 1, 2]], np.uint32))      # finite; overflows at scale 2
    px = [(6, 3), (28, 4), (9, 14)]                              # frame 1: pixel coordinates; p = (-64 X, -64 Y, 64 X - 64), r2 = -64
    neg = (np.array([[-64.0 * X, -64.0 * Y, 64.0 * X - 64.0] for X, Y in px], F32), np.array([[0, 1, 2]], np.uint32))
    K1 = KUNIT.copy()
    K1[2, 0] = 1.0
    assert_snapped(neg[0], [(16 * X, 16 * Y, 64.0 * X - 64.0) for X, Y in px], K=K1)
    meshes = [big.mesh(), twin.mesh(), near.mesh(), edge, neg]
    inst = [rr.instance(0, 0, head=False), rr.instance(0, 1)]
    bad = (float("nan"), INF, -INF)
    for j, v in enumerate(bad):
        t = [0.0, 0.0, 0.0]
        t[j] = v
        R = EYE.copy()
        R[j, j] = v
        inst += [rr.instance(0, 2, t=t), rr.instance(0, 2, R=R), rr.instance(0, 2, scale=v)]
    inst.append(rr.instance(0, 2, t=(0, 0, INF)))
    Rsum = EYE.copy()
    Rsum[0, 1] = -1.0                                             # p.x = inf - inf
    inst += [rr.instance(0, 3, scale=2.0), rr.instance(0, 3, scale=-2.0), rr.instance(0, 3, R=Rsum, scale=2.0)]
    inst += [rr.instance(0, 2, t=(1, 1, 100), scale=0.0), rr.instance(0, 2, scale=-1.0)]
    inst.append(rr.instance(1, 4))

    def reach(cs):
        assert [(r["instance"], r["frame"]) for r in cs["records"]] == [(0, 0), (len(inst) - 1, 1)]
        r0 = cs["records"][0]
        assert {abs(v) for v in r0["x"] + r0["y"]} == {BAND} and r0["covered"] == w * h
        assert cs["dropped"]["guard"] == 1 and cs["dropped"]["area"] == 1 and cs["dropped"]["z"] + cs["dropped"]["nonfinite"] == 14, cs["dropped"]
        assert sum(cs["dropped"].values()) == len(inst) - 2 and cs["records"][1]["covered"] > 20
        assert set(np.unique(cs["depth"][0]).tolist()) == {1024} and cs["depth"][1].max() > 0

    return [case("guard_band", meshes, inst, 2, w, h, reach, K=np.stack([KUNIT, K1]))]


# ------------------------------------------------------------------ frame_shapes
def shape_case(label, w, h, n, sensor=None, empty_last=True, scene=None):
    """n frames of w x h: in each but the last a triangle over the whole frame (no head), and one-pixel head triangles in the four
    corners and in the middle of the last row and column; the last frame stays empty."""
    cover = Soup().tri((-16, -16), (16 * (2 * w + 4), -16), (-16, 16 * (2 * h + 4)), (2048.0, 2304.0, 2176.0))
    dots = Soup()
    spots = sorted({(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h - 1), (w - 1, h // 2)})
    for k, (c, r) in enumerate(spots):
        dots.corner(c, r, 1, 1, 1000.0 + k)
    meshes = [cover.mesh(), dots.mesh()]
    drawn = n - 1 if empty_last else n
    inst = [rr.instance(f, m, head=m == 1) for f in range(drawn) for m in (0, 1)]
    tiles = n * -(-w // DH_RT_W) * -(-h // DH_RT_H)

    def reach(cs):
        assert cs["n_tiles"] == tiles and not cs["dropped"]
        assert (cs["depth"][:drawn] > 0).all() and not cs["depth"][drawn:].any()
        for c, r in spots:
            assert cs["mask"][:drawn, r, c].all() and (cs["cover"][:drawn, r, c] == 2).all()
        assert cs["mask"][:drawn].sum() == drawn * len(spots)

    return case(label, meshes, inst, n, w, h, reach, sensor=sensor, scene=scene)


SHAPES = [(1, 1, 257), (7, 3, 65), (8, 1, 9), (9, 17, 2), (63, 15, 2), (64, 16, 2), (65, 17, 2), (72, 16, 2), (128, 32, 2), (16384, 1, 2), (1, 16384, 2)]


def frame_shapes():
    """The eleven sizes; tile totals of 257, 65, 9 and (a single frame of 64 x 16, the one case without an empty frame) 1 among
    them.  7 x 3 and 65 x 17 (narrow stores) again with noise 2 and 5 % holes, seeds 0 and 2^64 - 1; 9 x 17 with a hole
    probability of 2^-53 and 63 x 15 with 1 - 2^-53."""
    out = [shape_case("frame_shapes-%dx%dx%d" % (w, h, n), w, h, n) for w, h, n in SHAPES]
    out.append(shape_case("frame_shapes-64x16x1", 64, 16, 1, empty_last=False))
    out.append(shape_case("frame_shapes-7x3x65-sensor", 7, 3, 65, sensor={"noise": 2, "holes": 0.05, "seed": 0}, scene="frame_shapes-7x3x65"))
    out.append(shape_case("frame_shapes-65x17x2-sensor", 65, 17, 2, sensor={"noise": 2, "holes": 0.05, "seed": (1 << 64) - 1}, scene="frame_shapes-65x17x2"))
    out.append(shape_case("frame_shapes-9x17x2-holes-min", 9, 17, 2, sensor={"noise": 0, "holes": 2.0 ** -53, "seed": 3}, scene="frame_shapes-9x17x2"))
    out.append(shape_case("frame_shapes-63x15x2-holes-max", 63, 15, 2, sensor={"noise": 0, "holes": 1.0 - 2.0 ** -53, "seed": 4}, scene="frame_shapes-63x15x2"))
    totals = {c["n"] * -(-c["w"] // DH_RT_W) * -(-c["h"] // DH_RT_H) for c in out}
    assert {1, 9, 65, 257} <= totals
    return out


def all_dropped():
    """A call in which every triangle is dropped (behind the camera, not finite, outside the guard band, off the frame): nothing
    reaches a tile list."""
    g = guard_band()[0]
    keep = g["instances"][1:-1]
    off = Soup().corner(40, 3, 5, 5, 100.0)                       # right of a 32-pixel frame: no pixel
    meshes = g["meshes"] + [off.mesh()]
    inst = keep + [rr.instance(1, len(meshes) - 1)]

    def reach(cs):
        assert not cs["records"] and not cs["tile_count"].any() and sum(cs["dropped"].values()) == len(inst) and cs["dropped"]["nopixel"] == 1

    return case("all_dropped", meshes, inst, 2, 32, 16, reach)


FAMILIES = {"centres_on_edges": centres_on_edges, "tile_seams": tile_seams, "small_big_split": small_big_split, "deep_lists": deep_lists,
            "depth_range": depth_range, "guard_band": guard_band, "frame_shapes": frame_shapes}


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(FAMILIES[family]())


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case of every family, and the all-dropped call, by label."""
    out = {c["label"]: c for f in FAMILIES for c in cases(f)}
    out["all_dropped"] = all_dropped()
    return out


LABELS = ["centres_on_edges", "tile_seams", "small_big_split", "deep_lists", "depth_range", "depth_range-noise3", "depth_range-noise65535",
          "guard_band"] + ["frame_shapes-%dx%dx%d" % s for s in SHAPES] + \
         ["frame_shapes-64x16x1", "frame_shapes-7x3x65-sensor", "frame_shapes-65x17x2-sensor", "frame_shapes-9x17x2-holes-min",
          "frame_shapes-63x15x2-holes-max", "all_dropped"]
