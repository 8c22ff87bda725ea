"""tests/render_ref.py (the rendering rule of DESIGN.md section 17) against cases whose answers are known on paper.  Exact
conditions, no tolerance, except the slanted plane, whose +-1 is derived there."""
import numpy as np

import render_ref as rr

W, H = 64, 48
K = np.array([[100.0, 0.0, 32.0], [0.0, 100.0, 24.0], [0.0, 0.0, 1.0]], np.float32)     # pixel = 100 * x / z + centre: exact at z = 100, 200, 400
QUAD = (np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))


def quad_at(z, half, frame=0, head=True, centre=(0.0, 0.0)):
    return rr.instance(frame, 0, None, (centre[0], centre[1], z), scale=half, head=head)


def test_axis_aligned_quad_gives_its_depth_on_exactly_the_centres_inside():
    # half 21.3 mm at z = 200: x from 32 - 10.65 to 32 + 10.65 pixels; snapped to 1/16: 21.375 .. 42.625 (341.5 -> 342, 682.5 -> 682 by
    # floor(v + 0.5)); centres x + 0.5 inside [21.375, 42.625): x = 21 .. 42, the right and bottom edges own nothing
    d, m = rr.render([QUAD], [quad_at(200.0, 21.3)], 1, W, H, K)
    sx, _ = rr.project(K, rr.transform(QUAD[0], np.eye(3, dtype=np.float32), np.float32([0, 0, 200]), 21.3))
    x0, x1 = int(sx.min()), int(sx.max())
    want = np.zeros((H, W), bool)
    xs = [x for x in range(W) if x0 <= 16 * x + 8 < x1]
    ys = [y for y in range(H) if x0 - 128 <= 16 * y + 8 < x1 - 128]          # (the centre row is 8 pixels = 128 sixteenths higher)
    want[np.ix_(ys, xs)] = True
    assert xs == list(range(21, 43)) and ys == list(range(13, 35))
    assert np.array_equal(d[0] > 0, want) and np.array_equal(m[0] > 0, want)
    assert (d[0][want] == 200).all()
    # a left / top edge exactly on the centres owns them, a right / bottom edge does not: half 21 mm at z = 200 puts the edges at
    # 21.5 and 42.5 exactly
    d, _ = rr.render([QUAD], [quad_at(200.0, 21.0)], 1, W, H, K)
    assert np.array_equal(np.flatnonzero((d[0] > 0).any(axis=0)), np.arange(21, 42))
    assert np.array_equal(np.flatnonzero((d[0] > 0).any(axis=1)), np.arange(13, 34))


def _coverage_count(mesh, ins, w=W, h=H):
    """How many triangles of the mesh cover each pixel: every triangle drawn alone."""
    count = np.zeros((h, w), int)
    for tri in mesh[1]:
        d, _ = rr.render([(mesh[0], tri.reshape(1, 3))], [ins], 1, w, h, K)
        count += d[0] > 0
    return count


def test_shared_edges_cover_every_pixel_exactly_once():
    # the quad's diagonal runs through pixel centres (half 21 at z = 200: corners on half pixels)
    for half in (21.0, 21.3, 17.77):
        ins = quad_at(200.0, half)
        count = _coverage_count(QUAD, ins)
        whole, _ = rr.render([QUAD], [ins], 1, W, H, K)
        assert count.max() == 1 and np.array_equal(count == 1, whole[0] > 0)
    # a fan of twelve triangles round one vertex that sits exactly on a pixel centre, both windings mixed
    ang = np.arange(12) * (2 * np.pi / 12)
    verts = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(ang), np.sin(ang), np.zeros(12)], axis=1)]).astype(np.float32)
    tris = np.array([[0, 1 + i, 1 + (i + 1) % 12] if i % 2 else [0, 1 + (i + 1) % 12, 1 + i] for i in range(12)], np.uint32)
    ins = rr.instance(0, 0, None, (1.0, 1.0, 200.0), scale=30.0)            # centre at pixel 32.5, 24.5
    count = _coverage_count((verts, tris), ins)
    assert count.max() == 1 and count[24, 32] == 1 and count.sum() > 600
    inner = np.hypot(*np.meshgrid(np.arange(W) - 32, np.arange(H) - 24)) < 13.5          # inside the fan's inscribed circle
    assert (count[inner] == 1).all()


def test_occlusion_and_the_tie():
    head = quad_at(400.0, 40.0)                                  # 10 pixels half size at z = 400
    front = quad_at(390.0, 20.0, head=False, centre=(10.0, 0.0))
    behind = quad_at(410.0, 80.0, head=False)
    d, m = rr.render([QUAD], [head, front, behind], 1, W, H, K)
    only_head, _ = rr.render([QUAD], [head], 1, W, H, K)
    only_front, _ = rr.render([QUAD], [front], 1, W, H, K)
    hf, ff = only_head[0] > 0, only_front[0] > 0
    assert (hf & ff).any() and (hf & ~ff).any()
    assert (d[0][ff] == 390).all() and not m[0][ff].any()                 # in front: the head is gone from depth and mask
    assert (d[0][hf & ~ff] == 400).all() and m[0][hf & ~ff].all()         # behind: the box loses
    assert (d[0][(d[0] > 0) & ~hf & ~ff] == 410).all()
    for order in ([True, False], [False, True]):                          # equal depth: the head wins, whatever the order
        d, m = rr.render([QUAD], [quad_at(400.0, 40.0, head=o) for o in order], 1, W, H, K)
        assert np.array_equal(m[0] > 0, hf) and (d[0][hf] == 400).all()


def test_dropped_triangles_draw_nothing():
    tri = (np.array([[0, 0, 0], [30, 0, 0], [0, 30, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
    assert rr.render([tri], [rr.instance(0, 0, None, (0, 0, 200.0))], 1, W, H, K)[0].any()
    assert not rr.render([tri], [rr.instance(0, 0, None, (0, 0, 0.5))], 1, W, H, K)[0].any()           # behind z = 1
    assert not rr.render([tri], [rr.instance(0, 0, None, (0, 0, -200.0))], 1, W, H, K)[0].any()
    one_behind = (np.array([[0, 0, 0], [30, 0, 0], [0, 30, -199.5]], np.float32), tri[1])
    assert not rr.render([one_behind], [rr.instance(0, 0, None, (0, 0, 200.0))], 1, W, H, K)[0].any()  # dropped whole, not clipped
    flat = (np.array([[0, 0, 0], [10, 10, 0], [20, 20, 0]], np.float32), tri[1])
    assert not rr.render([flat], [rr.instance(0, 0, None, (0, 0, 200.0))], 1, W, H, K)[0].any()        # zero area
    tiny = (np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0]], np.float32), tri[1])
    assert not rr.render([tiny], [rr.instance(0, 0, None, (0, 0, 200.0))], 1, W, H, K)[0].any()        # zero area after the snap
    # the guard band: 2^20 sixteenths = 65536 pixels.  A triangle over the whole frame with a vertex past it is dropped ...
    big = (np.array([[-100, -100, 0], [140000, -100, 0], [-100, 140000, 0]], np.float32), tri[1])
    assert not rr.render([big], [rr.instance(0, 0, None, (0, 0, 200.0))], 1, W, H, K)[0].any()
    # ... and one just inside it is drawn
    ok = (np.array([[-100, -100, 0], [130000, -100, 0], [-100, 130000, 0]], np.float32), tri[1])
    assert (rr.render([ok], [rr.instance(0, 0, None, (0, 0, 200.0))], 1, W, H, K)[0] == 200).all()
    nan = (np.array([[0, 0, 0], [30, 0, 0], [0, 30, 0]], np.float32), tri[1])
    assert not rr.render([nan], [rr.instance(0, 0, None, (0, np.inf, 200.0))], 1, W, H, K)[0].any()   # a coordinate that is not finite


def test_slanted_plane_matches_the_ray_plane_depth():
    """A quad turned 35 degrees about y and 20 about x.  The analytic depth under pixel centre (x + 0.5, y + 0.5) is the ray's
    intersection with the plane through the quad.  The renderer differs from it in two ways only.  Its vertices are f32 and
    snapped to 1/16 pixel while they keep their depth: a corner moves by up to 1/32 pixel each way, and with a pixel 4 mm wide
    at 400 mm and the plane 38 degrees off the image plane (depth gradient under tan(38 deg) * 4 = 3.2 mm per pixel) that shifts
    the interpolated plane by under 3.2 * sqrt(2) / 32 = 0.15 mm.  And the final rounding to an integer adds at most 0.5.  Both
    together stay below the +-1 asserted at every covered pixel."""
    a, b = np.radians(35.0), np.radians(20.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R = Rx @ Ry
    t = np.array([3.0, -2.0, 400.0])
    d, m = rr.render([QUAD], [rr.instance(0, 0, R, t, scale=60.0)], 1, W, H, K)
    ys, xs = np.nonzero(d[0])
    assert len(xs) > 300 and m[0].sum() == len(xs)
    nrm = R[:, 2]                                                          # the plane: nrm . (p - t) = 0
    ray = np.stack([(xs + 0.5 - 32.0) / 100.0, (ys + 0.5 - 24.0) / 100.0, np.ones(len(xs))], axis=1)
    z = (nrm @ t) / (ray @ nrm)
    assert z.max() - z.min() > 40                                          # it is slanted
    err = np.abs(d[0][ys, xs].astype(np.float64) - z)
    assert err.max() <= 1.0, err.max()


def test_sensor_model_draws_are_the_splitmix_stream():
    from depthhead_amd import synth
    assert np.array_equal(rr.splitmix_at(1234, np.arange(10)), synth.SplitMix(1234).u64(10))
    keys = rr.render_keys([QUAD], [quad_at(400.0, 80.0)], 2, W, H, K)
    clean, mask = rr.resolve(keys)
    assert np.array_equal(rr.resolve(keys, 0, 0.0, 5)[0], clean)
    d, m = rr.resolve(keys, 3, 0.0, 5)
    fg = clean > 0
    u = synth.SplitMix(5).u64(2 * keys.size).reshape(-1, 2)
    want = np.where(fg.ravel(), 400 + (u[:, 0] % np.uint64(7)).astype(np.int64) - 3, 0)
    assert np.array_equal(d.ravel(), want) and np.array_equal(m, mask) and not d[1].any()
    d, m = rr.resolve(keys, 0, 0.25, 5)
    holes = (u[:, 1] >> np.uint64(11)) < np.uint64(2 ** 51)
    assert np.array_equal(d.ravel() == 0, ~fg.ravel() | holes) and np.array_equal(m, mask)
    assert not rr.resolve(keys, 0, 1.0, 5)[0].any()
