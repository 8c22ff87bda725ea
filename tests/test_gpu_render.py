"""The renderer on the GPU against its restatement (tests/render_ref.py): depth frames and masks bit for bit
on every pixel of every frame -- head meshes at seeded poses, triangles larger than the frame and across each edge, frame sizes
that are no multiple of the 64 x 16 tile (and one whose width is no multiple of the 8-pixel store), empty frames, sixteen
instances with mutual occlusion, the depth tie, camera tables, the sensor model, the device twins and a renderer reused with a
smaller and then a larger batch."""
import functools

import numpy as np
import pytest

import render_ref as rr
from depthhead_amd import render, synth

pytestmark = pytest.mark.gpu

SIZES = [(96, 96), (128, 112), (160, 120), (320, 240), (640, 480), (100, 50)]


@functools.lru_cache(maxsize=None)
def head():
    v, t = synth.head_mesh(2)          # 162 vertices, 320 triangles: every path of the kernels at a quarter of the reference's time
    v.setflags(write=False); t.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def torso():
    v, t = synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))
    v.setflags(write=False); t.setflags(write=False)
    return v, t


QUAD = (np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))
TRI = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32))
MESHES = (head, torso, lambda: QUAD, lambda: TRI)


def host_meshes():
    return [m() for m in MESHES]


@pytest.fixture(scope="module")
def gpu():
    ms = [render.Mesh(*m()) for m in MESHES]
    rd = render.Renderer()
    yield ms, rd
    rd.close()
    for m in ms:
        m.close()


def to_gpu(items):
    return render.instances([(i["frame"], i["mesh"], i["R"], i["t"], float(i["scale"]), bool(i["flags"])) for i in items])


def check(gpu, items, n, w, h, K, keys=None, **sensor):
    """Render on the GPU and compare every pixel with the restatement (keys: its key image when the caller has it already)."""
    ms, rd = gpu
    frames, masks = rd.render(ms, to_gpu(items), n, w, h, K, **sensor)
    want_f, want_m = rr.resolve(rr.render_keys(host_meshes(), items, n, w, h, K) if keys is None else keys, **sensor)
    assert frames.shape == want_f.shape and frames.dtype == np.uint16 and masks.dtype == np.uint8
    bad = np.argwhere(frames != want_f)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), frames[tuple(bad[0])], want_f[tuple(bad[0])])
    assert np.array_equal(masks, want_m), np.argwhere(masks != want_m)[:5].tolist()
    return frames, masks


def head_scene(n, w, h, seed, with_torso=True):
    """n frames: a head at a seeded pose at 600 - 1300 mm and its torso box; the last frame stays empty when n > 2."""
    u = synth.SplitMix(seed).uniform(6 * n).reshape(n, 6)
    K = synth.default_intrinsic(w, h)
    items = []
    for f in range(n - 1 if n > 2 else n):
        z = 600.0 + 700.0 * u[f, 0]
        pos = ((w * (0.2 + 0.6 * u[f, 1]) - w / 2) * z / K[0, 0], (h * (0.2 + 0.6 * u[f, 2]) - h / 2) * z / K[1, 1], z)
        rot = (20 * u[f, 3] - 10, 80 * u[f, 4] - 40, 40 * u[f, 5] - 20)
        items.append(rr.instance(f, 0, render.euler_to_matrix(rot), pos))
        if with_torso:
            items.append(rr.instance(f, 1, None, pos, head=False))
    return items, K


@functools.lru_cache(maxsize=None)
def scene_keys(n, w, h, seed):
    """The restatement's key image of head_scene(n, w, h, seed): computed once, shared, read-only."""
    items, K = head_scene(n, w, h, seed)
    keys = rr.render_keys(host_meshes(), items, n, w, h, K)
    keys.setflags(write=False)
    return keys


@pytest.mark.parametrize("w,h", SIZES)
def test_heads_at_seeded_poses(gpu, w, h):
    items, K = head_scene(3, w, h, 1000 + w)
    frames, masks = check(gpu, items, 3, w, h, K)
    assert masks[:2].any(axis=(1, 2)).all() and (frames[:2] > 0).sum() > masks[:2].sum()      # heads and torsos were drawn
    assert not frames[2].any() and not masks[2].any()                                           # the frame with no instance


def test_no_instance_at_all(gpu):
    ms, rd = gpu
    frames, masks = rd.render(ms, to_gpu([]), 2, 160, 120, synth.default_intrinsic(160, 120))
    assert frames.shape == (2, 120, 160) and not frames.any() and not masks.any()


def test_large_and_clipped_triangles(gpu):
    """Frame 0: one triangle larger than the frame (the quad scaled far past it is two).  Frames 1 - 4: a triangle partly off the
    left, right, top and bottom edge.  Frame 5: a triangle that covers the frame and a head in front of it."""
    w, h = 160, 120
    K = synth.default_intrinsic(w, h)
    f = float(K[0, 0])
    items = [rr.instance(0, 3, None, (-3000.0, -2500.0, 1000.0), scale=9000.0, head=False)]
    px = 1000.0 / f                               # mm per pixel at 1 m
    for i, (cx, cy) in enumerate([(-10, 60), (150, 40), (70, -12), (90, 110)]):
        items.append(rr.instance(1 + i, 3, render.euler_to_matrix((10 * i, 5, -7)), ((cx - w / 2) * px, (cy - h / 2) * px, 1000.0), scale=37.0 * px))
    items.append(rr.instance(5, 3, None, (-3000.0, -2500.0, 1200.0), scale=9000.0, head=False))
    items.append(rr.instance(5, 0, render.euler_to_matrix((0, 25, 10)), (10.0, -5.0, 800.0)))
    frames, masks = check(gpu, items, 6, w, h, K)
    assert (frames[0] == 1000).all() and not masks[0].any()
    for i in range(1, 5):
        assert 0 < masks[i].sum() < 37 * 37 / 2
    assert (frames[5] > 0).all() and 0 < masks[5].sum() < w * h


def test_sixteen_instances_and_two_heads_occluding_each_other(gpu):
    w, h = 320, 240
    K = synth.default_intrinsic(w, h)
    u = synth.SplitMix(77).uniform(16 * 5).reshape(16, 5)
    items = [rr.instance(0, 0, render.euler_to_matrix((0, 30, 0)), (-40.0, 0.0, 800.0)),
             rr.instance(0, 0, render.euler_to_matrix((0, -30, 0)), (40.0, 10.0, 830.0))]        # interpenetrating heads
    for i in range(2, 16):
        pos = (600 * u[i, 0] - 300, 400 * u[i, 1] - 200, 700 + 500 * u[i, 2])
        items.append(rr.instance(0, i % 2, render.euler_to_matrix((0, 90 * u[i, 3] - 45, 40 * u[i, 4] - 20)), pos, head=i % 2 == 0))
    check(gpu, items, 1, w, h, K)


def test_head_wins_the_equal_depth_tie(gpu):
    w, h = 96, 96
    K = synth.default_intrinsic(w, h)
    for order in ((True, False), (False, True)):
        items = [rr.instance(0, 2, None, (0.0, 0.0, 900.0), scale=150.0, head=hd) for hd in order]
        frames, masks = check(gpu, items, 1, w, h, K)
        assert masks.sum() == (frames == 900).sum() > 0


def test_camera_table_with_a_matrix_per_frame(gpu):
    from depthhead_amd.tracking import Cameras
    w, h, n = 160, 120, 3
    items, K = head_scene(2, w, h, 5)
    items.append(rr.instance(2, 0, render.euler_to_matrix((5, -20, 0)), (0.0, 20.0, 1000.0)))
    Ks = np.stack([K, K * np.float32(1.0), K]).astype(np.float32)
    Ks[1, 0, 0] *= 1.3; Ks[1, 1, 1] *= 0.8; Ks[1, 0, 2] += 11.5
    Ks[2, 0, 1] = 3.0; Ks[2, 2, 0] = 1e-4                      # a matrix that is no pinhole
    ms, rd = gpu
    want_f, want_m = rr.render(host_meshes(), items, n, w, h, Ks)
    with Cameras(Ks) as cams:
        frames, masks = rd.render(ms, to_gpu(items), n, w, h, cams)
    assert np.array_equal(frames, want_f) and np.array_equal(masks, want_m)
    one_f, one_m = rd.render(ms, to_gpu(items), n, w, h, K)
    assert np.array_equal(one_f[0], frames[0]) and not np.array_equal(one_f[1], frames[1])


@pytest.mark.parametrize("noise,holes", [(0, 0.0), (2, 0.02), (0, 1.0)])
def test_sensor_model(gpu, noise, holes):
    w, h = 160, 120
    items, K = head_scene(3, w, h, 31)
    frames, masks = check(gpu, items, 3, w, h, K, keys=scene_keys(3, w, h, 31), noise=noise, holes=holes, seed=0xC0FFEE + noise)
    clean, clean_m = rr.resolve(scene_keys(3, w, h, 31))
    assert np.array_equal(masks, clean_m)                     # holes leave the mask alone
    if holes == 1.0:
        assert not frames.any() and masks.any()
    elif noise:
        fg = clean > 0
        assert 0.005 < ((frames == 0) & fg).sum() / fg.sum() < 0.04
        kept = fg & (frames > 0)
        assert np.abs(frames[kept].astype(int) - clean[kept].astype(int)).max() == noise
    else:
        assert np.array_equal(frames, clean)


def _np(t):
    import torch
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype != torch.uint8 else t.numpy()


def test_device_twins_are_byte_identical(gpu):
    import torch
    from depthhead_amd.tracking import Cameras
    ms, rd = gpu
    w, h, n = 160, 120, 3
    items, K = head_scene(n, w, h, 31)
    inst = to_gpu(items)
    for sensor in ({}, {"noise": 2, "holes": 0.02, "seed": 9}):
        hf, hm = rd.render(ms, inst, n, w, h, K, **sensor)
        df, dm = rd.render(ms, inst, n, w, h, K, device_out=True, **sensor)
        torch.cuda.synchronize()
        assert np.array_equal(_np(df), hf) and np.array_equal(_np(dm), hm)
        with Cameras(np.tile(K.reshape(1, 9), (n, 1))) as cams:
            cf, cm = rd.render(ms, inst, n, w, h, cams, device_out=True, **sensor)
            f2, _ = rd.render(ms, inst, n, w, h, cams, device_out=True, masks=False, **sensor)
            torch.cuda.synchronize()
        assert np.array_equal(_np(cf), hf) and np.array_equal(_np(cm), hm) and np.array_equal(_np(f2), hf)


def test_smaller_then_larger_batch_in_one_renderer(gpu):
    """Stale records, counters and lists: a renderer that drew a small batch, then a larger one, then the small one again."""
    ms, _ = gpu
    small, K = head_scene(1, 96, 96, 3)
    large, K2 = head_scene(4, 320, 240, 4)
    with render.Renderer() as rd:
        for items, n, w, h, k, seed in ((small, 1, 96, 96, K, 3), (large, 4, 320, 240, K2, 4), (small, 1, 96, 96, K, 3)):
            check((ms, rd), items, n, w, h, k, keys=scene_keys(n, w, h, seed))
