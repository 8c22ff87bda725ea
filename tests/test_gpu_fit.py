"""The fit on the GPU against its restatement (tests/fit_ref.py): R, t and every field of the record of
every instance byte for byte -- no tolerance, no instance left out.  Heads at seeded poses from far and near starts, a frame
whose width is no multiple of 8 with models across every edge, twelve instances over five frames (one empty, one with two
heads), models of 1, 257 and 2562 points (the workgroup's stride edge and the streaming path past the LDS budget), schedules
without coarse or without any steps, both early exits on a head scene, the FEW_POINTS and SINGULAR exits, a camera table with a matrix that is no pinhole, the
device twins chained after a device render on one stream, a fitter reused with a smaller, a larger and the smaller batch
again, and two runs of the same call.  The scenes here are rendered with seeded noise and random poses, so no point lands ON a
compare of the correspondence; tests/test_gpu_fit_edges.py holds this and every other entry point of the fit family to points
placed on each compare and one step to either side of it (tests/fit_edges.py)."""
import functools

import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import render_ref as rr
from gpu_kit import fit_models, same_records
from depthhead_amd import _lib, fit, render, synth

pytestmark = pytest.mark.gpu

INST, REC = _lib.RENDER_INSTANCE_DTYPE, _lib.FIT_RECORD_DTYPE


@functools.lru_cache(maxsize=None)
def host_models():
    """0: head_mesh(2), 162 points.  1: one point.  2: 257 points of head_mesh(3).  3: head_mesh(4), 2562 points, above the
    LDS staging budget of 1024.  4: a plane of 81 points.  5 - 9: the first 255, 256, 1023, 1024 and 1025 points of head_mesh(4): either side of
    the workgroup's 256 lanes and of the staging budget."""
    v2, _, n2 = fs.head(2)
    v3, _, n3 = fs.head(3)
    v4, _, n4 = fs.head(4)
    g = (np.arange(9) - 4.0) * 20.0
    x, y = np.meshgrid(g, g)
    plane = np.stack([x.ravel(), y.ravel(), np.zeros(81)], axis=1).astype(np.float32)
    pn = np.tile(np.array([0, 0, -1], np.float32), (81, 1))
    front = int(np.argmin(v2[:, 2]))                  # a point that faces the camera at the identity pose
    slices = tuple((v4[:k].copy(), n4[:k].copy()) for k in (255, 256, 1023, 1024, 1025))
    return ((v2, n2), (v2[front:front + 1].copy(), n2[front:front + 1].copy()), (v3[:257].copy(), n3[:257].copy()), (v4, n4), (plane, pn)) + slices


@pytest.fixture(scope="module")
def gpu():
    with fit_models(host_models()) as both:
        yield both


def instances(items):
    """A dh_render_instance array from (frame, model, R, t, scale) tuples; flags carry a pattern that must be copied through."""
    out = np.zeros(len(items), INST)
    for i, (frame, model, R, t, scale) in enumerate(items):
        out[i] = (frame, model, np.asarray(R, np.float32).reshape(9), np.asarray(t, np.float32).reshape(3), scale, 0x5A0000 + i)
    return out


def ref_params(prm):
    if prm is None:
        return fr.params()
    return fr.params(prm.coarse_iterations, prm.iterations, (prm.gate[0], prm.gate[1]), prm.lam, prm.min_points)


def expected(frames, Ks, inst, prm=None):
    """What the restatement gives for every instance: (instances, records) as the GPU lays them out."""
    Ks = np.asarray(Ks, np.float32)
    Ks = np.broadcast_to(Ks.reshape(-1, 3, 3), (len(frames), 3, 3)) if Ks.size == 9 else Ks.reshape(len(frames), 3, 3)
    out, rec = inst.copy(), np.zeros(len(inst), REC)
    for i, it in enumerate(inst):
        pts, nrm = host_models()[it["mesh"]]
        R, t, r = fr.fit(frames[it["frame"]], Ks[it["frame"]], pts, nrm, it["R"].reshape(3, 3), it["t"], it["scale"], ref_params(prm))
        out[i]["R"], out[i]["t"] = R.reshape(9), t
        rec[i] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"])
    return out, rec


def check(gpu, frames, K, inst, prm=None, K_gpu=None):
    ms, ft = gpu
    out, rec = ft.fit(frames, ms, inst, K if K_gpu is None else K_gpu, params=prm)
    want_out, want_rec = expected(frames, K, inst, prm)
    assert out.dtype == INST and rec.dtype == REC and len(out) == len(rec) == len(inst)
    same_records(rec, want_rec, "record")
    same_records(out, want_out, "instance")
    return out, rec


def starts(frame_index, seed, w, h, kinds=((90.0, 25.0), (20.0, 10.0)), model=0):
    _, _, pos, R = fs.scene(w, h, seed)
    return [(frame_index, model) + fs.start(seed + 31 * k, pos, R, off, deg) + (1.0,) for k, (off, deg) in enumerate(kinds)]


def test_one_instance_96x96(gpu):
    frame, K, pos, R = fs.scene(96, 96, 7100)
    out, rec = check(gpu, frame[None], K, instances(starts(0, 7100, 96, 96)[:1]))
    assert rec["status"][0] == fit.FIT_OK and rec["points"][0] >= 30 and rec["steps"][0] == 20
    assert np.linalg.norm(out["t"][0] - pos) < 10.0 and fs.geodesic_deg(out["R"][0].reshape(3, 3), R) < 15.0
    assert 0.3 < fit.rms(rec[0]) < 5.0
    assert out["flags"][0] == 0x5A0000 and out["scale"][0] == 1.0


def test_width_no_multiple_of_8_and_models_across_every_edge(gpu):
    """100 x 50: a rendered head in frame 0; in frame 1 a wall at 800 mm and a head model pushed half way out of the frame at
    each edge and each corner, so that points project to x < 0, x >= w, y < 0 and y >= h."""
    w, h = 100, 50
    frame, K, pos, R = fs.scene(w, h, 7200)
    wall = np.full((h, w), 800, np.uint16)
    items = starts(0, 7200, w, h)
    mm = 810.0 / float(K[0, 0])                         # mm per pixel at 810 mm
    for cx, cy in ((0, 25), (99.9, 25), (50, 0), (50, 49.9), (0, 0), (99.9, 49.9), (-30, 25), (50, 200)):
        items.append((1, 0, render.euler_to_matrix((0, 10, 5)), ((cx - K[0, 2]) * mm, (cy - K[1, 2]) * mm, 810.0), 0.25))
    out, rec = check(gpu, np.stack([frame, wall]), K, instances(items))
    assert (rec["points"][2:8] > 0).all()
    assert rec["status"][8] == rec["status"][9] == fit.FIT_FEW_POINTS and not rec["points"][8:].any()      # wholly outside the frame


@functools.lru_cache(maxsize=None)
def five_frames():
    """160 x 120: frames 0, 1 and 4 one head each, frame 2 two heads, frame 3 empty; twelve instances over them."""
    w, h = 160, 120
    K = synth.default_intrinsic(w, h)
    v, t, _ = fs.head()
    two = [rr.instance(0, 0, render.euler_to_matrix((4, -25, 8)), (-150.0, -10.0, 900.0)),
           rr.instance(0, 0, render.euler_to_matrix((-6, 30, -5)), (140.0, 20.0, 1000.0))]
    f2, _ = rr.render([(v, t)], two, 1, w, h, K, noise=2, holes=0.02, seed=5)
    frames = np.stack([fs.scene(w, h, 7000)[0], fs.scene(w, h, 7001)[0], f2[0], np.zeros((h, w), np.uint16), fs.scene(w, h, 7002)[0]])
    three = ((90.0, 25.0), (20.0, 10.0), (0.0, 0.0))
    items = starts(0, 7000, w, h, three) + starts(1, 7001, w, h, three)
    for k, head in enumerate(two):
        items.append((2, 0) + fs.start(40 + k, head["t"], head["R"], 60.0, 15.0) + (1.0,))
    items.append((2, 0) + fs.start(50, two[0]["t"], two[0]["R"], 15.0, 5.0) + (1.0,))
    items.append((3, 0, np.eye(3), (0.0, 0.0, 900.0), 1.0))
    items += starts(4, 7002, w, h)
    inst = instances(items)
    assert len(inst) == 12
    frames.setflags(write=False); inst.setflags(write=False)
    return frames, K, inst


@functools.lru_cache(maxsize=None)
def five_frames_expected():
    frames, K, inst = five_frames()
    out, rec = expected(frames, K, inst)
    out.setflags(write=False); rec.setflags(write=False)
    return out, rec


def test_twelve_instances_over_five_frames(gpu):
    ms, ft = gpu
    frames, K, inst = five_frames()
    out, rec = ft.fit(frames, ms, inst, K)
    want_out, want_rec = five_frames_expected()
    same_records(rec, want_rec, "record"); same_records(out, want_out, "instance")
    assert rec["status"][9] == fit.FIT_FEW_POINTS and rec["points"][9] == 0 and out[9].tobytes() == inst[9].tobytes()
    assert (np.delete(rec["status"], 9) == fit.FIT_OK).all() and (np.delete(rec["points"], 9) >= 30).all()
    assert np.linalg.norm(out["t"][6] - (-150.0, -10.0, 900.0)) < 10 and np.linalg.norm(out["t"][7] - (140.0, 20.0, 1000.0)) < 10


def test_two_runs_are_byte_identical(gpu):
    ms, ft = gpu
    frames, K, inst = five_frames()
    a = ft.fit(frames, ms, inst, K)
    b = ft.fit(frames, ms, inst, K)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    same_records(a[1], five_frames_expected()[1], "record")


@pytest.mark.parametrize("model,points", [(1, 1), (2, 257), (3, 2562), (5, 255), (6, 256), (7, 1023), (8, 1024), (9, 1025)])
def test_model_sizes(gpu, model, points):
    """One point (never enough: FEW_POINTS, but the last pass still counts it), 255, 256 and 257 points (the workgroup's 256-lane
    stride), 1023, 1024 and 1025 (the last model staged in LDS, m.n <= DH_FIT_LDS_POINTS, and the first streamed from global
    memory) and 2562 (far above it)."""
    ms, _ = gpu
    assert ms[model].info()[0] == points == len(host_models()[model][0])
    w, h = 160, 120
    frame, K, pos, R = fs.scene(w, h, 7000)
    items = starts(0, 7000, w, h, ((40.0, 10.0), (0.0, 0.0)), model=model)
    out, rec = check(gpu, frame[None], K, instances(items))
    if points == 1:
        assert (rec["status"] == fit.FIT_FEW_POINTS).all() and (rec["steps"] == 0).all() and (rec["points"] <= 1).all()
    else:
        assert (rec["status"] == fit.FIT_OK).all() and (rec["points"] > 60).all()
        assert np.linalg.norm(out["t"][0] - pos) < 10.0


@pytest.mark.parametrize("coarse,full", [(0, 14), (6, 0), (0, 0), (1, 1), (32, 32)])
def test_schedules(gpu, coarse, full):
    w, h = 160, 120
    frame, K, pos, R = fs.scene(w, h, 7003)
    prm = fit.fit_params(coarse_iterations=coarse, iterations=full)
    inst = instances(starts(0, 7003, w, h, ((20.0, 10.0),)))
    out, rec = check(gpu, frame[None], K, inst, prm)
    assert rec["steps"][0] <= coarse + full and rec["status"][0] == fit.FIT_OK
    if coarse + full == 0:                                            # only the last pass: the pose comes back as it went in
        assert out.tobytes() == inst.tobytes() and rec["points"][0] > 0 and rec["sum_r2_fixed"][0] > 0


def test_early_exit_from_the_coarse_phase_and_then_from_the_full_steps_on_a_head_scene(gpu):
    """The scene and the two starts of tests/test_fit_ref.py's test of the same name.  With the diagonal damped 1e8 times over
    every step on a rendered head is below 1e-6 mm: the first coarse step ends the coarse phase and the fit goes on to the full
    steps.  From the near start the first full step ends the fit (2 steps of 20); from the far start, which the coarse steps have
    not brought within the 25 mm gate, the first full pass finds no point (1 step, FEW_POINTS).  Damped 1e7 times the coarse
    steps are not yet below 1e-6 and all six run; the first full step is, and ends the fit (7 steps)."""
    w, h = 160, 120
    frame, K, pos, R = fs.scene(w, h, 7003)
    inst = instances(starts(0, 7003, w, h))
    out, rec = check(gpu, frame[None], K, inst, fit.fit_params(lam=1e8))
    assert rec["steps"].tolist() == [1, 2] and rec["status"].tolist() == [fit.FIT_FEW_POINTS, fit.FIT_OK] and rec["points"][1] >= 30
    out, rec = check(gpu, frame[None], K, inst, fit.fit_params(lam=1e7))
    assert rec["steps"].tolist() == [6, 7] and rec["status"].tolist() == [fit.FIT_FEW_POINTS, fit.FIT_OK]
    assert np.abs(out["t"] - inst["t"]).max() < 1e-3


def test_other_params(gpu):
    w, h = 160, 120
    frame, K, pos, R = fs.scene(w, h, 7004)
    inst = instances(starts(0, 7004, w, h))
    check(gpu, frame[None], K, inst, fit.fit_params(gate=(200.0, 40.0), lam=0.0, min_points=6))
    out, rec = check(gpu, frame[None], K, inst, fit.fit_params(gate=(4096.0, 4096.0), lam=0.5, min_points=60))
    check(gpu, frame[None], K, inst, fit.fit_params(coarse_iterations=3, iterations=5, gate=(0.5, 0.25)))


def test_start_so_far_off_that_the_first_pass_finds_too_few_points(gpu):
    w, h = 160, 120
    frame, K, pos, R = fs.scene(w, h, 7005)
    items = [(0, 0, R, pos + (0.0, 0.0, 400.0), 1.0),                  # every depth difference beyond the gate
             (0, 0, R, pos + (3000.0, 0.0, 0.0), 1.0),                 # outside the frame
             (0, 0, R, (0.0, 0.0, -500.0), 1.0),                       # behind the camera
             (0, 0, R, (1e30, -1e30, 1e30), 1.0)]
    inst = instances(items)
    out, rec = check(gpu, frame[None], K, inst)
    assert (rec["status"] == fit.FIT_FEW_POINTS).all() and (rec["steps"] == 0).all() and (rec["points"] == 0).all()
    assert out.tobytes() == inst.tobytes()


def test_singular_exit(gpu):
    """The plane of tests/test_fit_ref.py, turned a little, with lambda = 0: SINGULAR at the first step and the pose as it was;
    face-on the 1e-9 term carries it through."""
    w, h = 160, 120
    K = synth.default_intrinsic(w, h)
    wall = np.full((1, h, w), 800, np.uint16)
    inst = instances([(0, 4, render.euler_to_matrix((0, 4, 3)), (0.0, 0.0, 810.0), 1.0), (0, 4, np.eye(3), (0.0, 0.0, 810.0), 1.0)])
    out, rec = check(gpu, wall, K, inst, fit.fit_params(coarse_iterations=0, iterations=3, lam=0.0))
    assert rec["status"].tolist() == [fit.FIT_SINGULAR, fit.FIT_OK] and rec["steps"][0] == 0 and out[0].tobytes() == inst[0].tobytes()
    assert out["t"][1].tolist() == [0.0, 0.0, 800.0]
    check(gpu, wall, K, inst, fit.fit_params(lam=0.0))
    check(gpu, wall, K, inst)


def test_camera_table_with_a_matrix_that_is_no_pinhole(gpu):
    from depthhead_amd.tracking import Cameras
    ms, ft = gpu
    w, h, n = 160, 120, 3
    K = synth.default_intrinsic(w, h)
    Ks = np.stack([K, K, K]).astype(np.float32)
    Ks[1, 0, 0] *= 1.3; Ks[1, 1, 1] *= 0.8; Ks[1, 0, 2] += 11.5
    Ks[2, 0, 1] = 3.0; Ks[2, 2, 0] = 1e-4                             # a matrix that is no pinhole
    v, t, _ = fs.head()
    poses = [(render.euler_to_matrix((3, 20, -8)), (30.0, -10.0, 850.0)), (render.euler_to_matrix((-5, -30, 10)), (-60.0, 15.0, 1000.0)),
             (render.euler_to_matrix((8, 10, 15)), (10.0, 20.0, 900.0))]
    frames, _ = rr.render([(v, t)], [rr.instance(f, 0, R, p) for f, (R, p) in enumerate(poses)], n, w, h, Ks, noise=2, holes=0.02, seed=8)
    assert frames.any(axis=(1, 2)).all()
    inst = instances([(f, 0) + fs.start(60 + f, p, R, 50.0, 15.0) + (1.0,) for f, (R, p) in enumerate(poses)])
    with Cameras(Ks) as cams:
        out, rec = check(gpu, frames, Ks, inst, K_gpu=cams)
        with pytest.raises(_lib.DepthheadError) as ei:
            ft.fit(frames[:2], ms, inst[:2], cams)
        assert ei.value.code == -1 and "holds 3 cameras" in str(ei.value)
    assert (rec["status"] == fit.FIT_OK).all()
    for f, (R, p) in enumerate(poses):
        assert np.linalg.norm(out["t"][f] - p) < 10.0, f
    one, _ = ft.fit(frames, ms, inst, K)
    assert one[0].tobytes() == out[0].tobytes() and one[2].tobytes() != out[2].tobytes()


def test_device_twins_chained_after_a_device_render(gpu):
    """dh_render_depth_device and dh_fit_depth_device on one stream with no host copy or wait between them, against the host call
    on the same frames and against the restatement; then the camera-table twin."""
    import torch
    from depthhead_amd.tracking import Cameras
    ms, ft = gpu
    w, h, n = 160, 120, 3
    K = synth.default_intrinsic(w, h)
    v, t, _ = fs.head()
    bv, bt = fs.torso()
    items = []
    truth = []
    for f in range(2):                                                 # the last frame stays empty
        _, _, pos, R = fs.scene(w, h, 7006 + f)
        truth.append((pos, R))
        items += [(f, 0, R, pos, 1.0, True), (f, 1, np.eye(3), pos, 1.0, False)]
    inst = instances([(f, 0) + fs.start(70 + f, p, R, 60.0, 20.0) + (1.0,) for f, (p, R) in enumerate(truth)] + [(2, 0, np.eye(3), (0, 0, 900.0), 1.0)])
    stream = torch.cuda.Stream()
    with render.Mesh(v, t) as head, render.Mesh(bv, bt) as box, render.Renderer() as rd, Cameras(np.tile(K.reshape(1, 9), (n, 1))) as cams:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            frames, _ = rd.render([head, box], render.instances(items), n, w, h, K, noise=2, holes=0.02, seed=3, device_out=True, masks=False)
            d_out, d_rec = ft.fit(frames, ms, inst, K, device_out=True, stream=stream.cuda_stream)
            c_out, c_rec = ft.fit(frames, ms, inst, cams, device_out=True, stream=stream.cuda_stream)
        stream.synchronize()
        host = frames.cpu().view(torch.int16).numpy().view(np.uint16)
        got = [x.cpu().numpy().view(dt) for x, dt in ((d_out, INST), (d_rec, REC), (c_out, INST), (c_rec, REC))]
    h_out, h_rec = check(gpu, host, K, inst)
    same_records(got[0], h_out, "device instance"); same_records(got[1], h_rec, "device record")
    same_records(got[2], h_out, "camera device instance"); same_records(got[3], h_rec, "camera device record")
    assert h_rec["status"].tolist() == [fit.FIT_OK, fit.FIT_OK, fit.FIT_FEW_POINTS]
    for f, (p, R) in enumerate(truth):
        assert np.linalg.norm(h_out["t"][f] - p) < 10.0


def test_smaller_then_larger_then_smaller_batch_in_one_fitter(gpu):
    ms, _ = gpu
    small_f, small_K, _, _ = fs.scene(96, 96, 7100)
    small = instances(starts(0, 7100, 96, 96)[:1])
    frames, K, inst = five_frames()
    want_small = expected(small_f[None], small_K, small)
    with fit.Fitter() as ft:
        for _ in range(2):
            out, rec = ft.fit(small_f[None], ms, small, small_K)
            same_records(rec, want_small[1], "small record"); same_records(out, want_small[0], "small instance")
            out, rec = ft.fit(frames, ms, inst, K)
            same_records(rec, five_frames_expected()[1], "large record"); same_records(out, five_frames_expected()[0], "large instance")
        out, rec = ft.fit(small_f[None], ms, [], small_K)
        assert len(out) == 0 and len(rec) == 0


def test_refusals_that_need_a_model(gpu):
    ms, ft = gpu
    frame, K, pos, R = fs.scene(96, 96, 7100)
    radius = ms[0].info()[1]
    assert abs(radius - np.sqrt((host_models()[0][0].astype(np.float64) ** 2).sum(axis=1).max())) < 1e-9
    big = float(np.float32(4096.5 / radius))
    for scale in (big, -big):
        with pytest.raises(_lib.DepthheadError) as ei:
            ft.fit(frame[None], ms, instances([(0, 0, R, pos, scale)]), K)
        assert ei.value.code == -1 and "mm from its origin" in str(ei.value)
    check(gpu, frame[None], K, instances([(0, 0, R, pos, float(np.float32(4095.0 / radius)))]))
    with pytest.raises(_lib.DepthheadError):
        fit.Model(host_models()[0][0], host_models()[0][1] * np.float32(1.2))

