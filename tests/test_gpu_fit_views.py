"""The multi-view fit on the GPU against its restatement (tests/view_fit_ref.py): R, t and every field of
the record of every instance byte for byte -- no tolerance, no instance left out.  One view through the identity (also equal to
Fitter.fit), two and three views, first_cam > 0, a mask with gaps, bit 63 of a 64-camera table, models on either side of the
workgroup's stride and of the LDS budget, the term limit on either side, four instances over two rigs, schedules, both early
exits, min_points on either side of the summed count, a camera that is no pinhole, the host form against the _device twin
chained after a device render between guard bands, a fitter reused, two runs, a captured call, the refusals that need a
device, and view_instances_from_persons on a RigTracker step of a two-camera rig (shape and sanity, and the fit of what it makes)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import render_ref as rr
import view_fit_ref as vr
import view_fit_scenes as vs
from gpu_kit import fit_models, same_records
from depthhead_amd import _lib, fit, render, synth
from depthhead_amd.tracking import Cameras

pytestmark = pytest.mark.gpu

INST, REC = _lib.VIEW_INSTANCE_DTYPE, _lib.VIEW_FIT_RECORD_DTYPE
GUARD = 4096


@functools.lru_cache(maxsize=None)
def host_models():
    """0: head_mesh(2), 162 points.  1: one point.  2 - 4: the first 257, 1024 and 1025 points of head_mesh(4): past the
    workgroup's 256 lanes, the last model staged in LDS and the first streamed.  5, 6: 4096 and 4097 points (head_mesh(4) and
    its beginning again): either side of the term limit with 8 views.  7: a plane of 81 points."""
    v2, _, n2 = fs.head(2)
    v4, _, n4 = fs.head(4)
    front = int(np.argmin(v2[:, 2]))
    big = (np.concatenate([v4, v4[:1535]]), np.concatenate([n4, n4[:1535]]))
    g = (np.arange(9) - 4.0) * 20.0
    x, y = np.meshgrid(g, g)
    plane = np.stack([x.ravel(), y.ravel(), np.zeros(81)], axis=1).astype(np.float32)
    return ((v2, n2), (v2[front:front + 1].copy(), n2[front:front + 1].copy())) + tuple((v4[:k].copy(), n4[:k].copy()) for k in (257, 1024, 1025)) + \
        ((big[0][:4096].copy(), big[1][:4096].copy()), big, (plane, np.tile(np.array([0, 0, -1], np.float32), (81, 1))))


@pytest.fixture(scope="module")
def gpu():
    with fit_models(host_models()) as both:
        yield both


def instances(items):
    """A dh_view_instance array from (first_cam, model, views, R, t, scale) tuples; flags carry a pattern to be copied through."""
    out = np.zeros(len(items), INST)
    for i, (first, model, views, R, t, scale) in enumerate(items):
        out[i] = (first, model, views, np.asarray(R, np.float32).reshape(9), np.asarray(t, np.float32).reshape(3), scale, 0x5A0000 + i)
    return out


def ref_params(prm):
    if prm is None:
        return fr.params()
    return fr.params(prm.coarse_iterations, prm.iterations, (prm.gate[0], prm.gate[1]), prm.lam, prm.min_points)


def expected(frames, Ks, V, u, inst, prm=None):
    out, rec = inst.copy(), np.zeros(len(inst), REC)
    for i, it in enumerate(inst):
        pts, nrm = host_models()[it["model"]]
        R, t, r = vr.fit(frames, Ks, V, u, it["first_cam"], it["views"], pts, nrm, it["R"].reshape(3, 3), it["t"], it["scale"], ref_params(prm))
        out[i]["R"], out[i]["t"] = R.reshape(9), t
        rec[i] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"], r["views_used"])
    return out, rec


def check(gpu, frames, Ks, V, u, inst, prm=None):
    ms, ft = gpu
    with Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        assert views.info() == (len(Ks), 0)
        out, rec = ft.fit_views(frames, ms, inst, views, params=prm)
    want_out, want_rec = expected(frames, Ks, V, u, inst, prm)
    assert out.dtype == INST and rec.dtype == REC and len(out) == len(rec) == len(inst)
    same_records(rec, want_rec, "record")
    same_records(out, want_out, "instance")
    return out, rec


def world_start(seed, pos, R, offset=90.0, deg=25.0):
    return vs.start(seed, pos, R, offset, deg)


def test_one_view_through_the_identity_96x96_is_also_the_single_view_fit(gpu):
    ms, ft = gpu
    frame, K, pos, R = fs.scene(96, 96, 7100)
    R0, t0 = fs.start(7100, pos, R, 90.0, 25.0)
    eye, zero = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)
    out, rec = check(gpu, frame[None], K[None], eye, zero, instances([(0, 0, 1, R0, t0, 1.0)]))
    assert rec["status"][0] == fit.FIT_OK and rec["points"][0] >= 30 and rec["steps"][0] == 20 and rec["views_used"][0] == 1
    assert out["flags"][0] == 0x5A0000 and out["scale"][0] == 1.0
    single = np.zeros(1, _lib.RENDER_INSTANCE_DTYPE)
    single[0] = (0, 0, R0.reshape(9), t0, 1.0, 0)
    with Cameras(K[None]) as cams:
        s_out, s_rec = ft.fit(frame[None], ms, single, cams)
    assert s_out["R"].tobytes() == out["R"].tobytes() and s_out["t"].tobytes() == out["t"].tobytes()
    assert s_rec.tobytes() == rec.tobytes()[:24]


@pytest.mark.parametrize("n_views", [2, 3])
def test_two_and_three_views_96x96(gpu, n_views):
    frames, Ks, V, u, pos, R = vs.scene(7100, n_views, 96, 96)
    out, rec = check(gpu, frames, Ks, V, u, instances([(0, 0, (1 << n_views) - 1) + world_start(7100, pos, R) + (1.0,)]))
    assert rec["status"][0] == fit.FIT_OK and rec["views_used"][0] == (1 << n_views) - 1 and rec["steps"][0] == 20
    assert np.linalg.norm(out["t"][0] - pos) < 10.0 and vs.geodesic_deg(out["R"][0].reshape(3, 3), R) < 15.0


def padded(seed, n_views, w, h, before, after):
    """The scene's cameras with `before` empty cameras (V = I, u = 0) in front and `after` behind."""
    frames, Ks, V, u, pos, R = vs.scene(seed, n_views, w, h)
    n = before + n_views + after
    F, KK = np.zeros((n, h, w), np.uint16), np.ascontiguousarray(np.broadcast_to(Ks[0], (n, 3, 3)))
    VV, uu = np.ascontiguousarray(np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3))), np.zeros((n, 3), np.float32)
    F[before:before + n_views], VV[before:before + n_views], uu[before:before + n_views] = frames, V, u
    return F, KK, VV, uu, pos, R


def test_first_cam_above_zero_and_a_mask_with_gaps(gpu):
    frames, Ks, V, u, pos, R = padded(7101, 3, 96, 96, 2, 1)
    start = world_start(7101, pos, R, 40.0, 15.0)
    items = [(2, 0, 0b111) + start + (1.0,), (2, 0, 0b101) + start + (1.0,), (1, 0, 0b1010) + start + (1.0,), (4, 0, 0b1) + start + (1.0,),
             (0, 0, 0b11101) + start + (1.0,)]
    out, rec = check(gpu, frames, Ks, V, u, instances(items))
    assert rec["views_used"].tolist() == [0b111, 0b101, 0b1010, 0b1, 0b11100] and (rec["status"] == fit.FIT_OK).all()
    assert out[1].tobytes()[16:] != out[0].tobytes()[16:] and out["R"][2].tobytes() == out["R"][1].tobytes()      # cameras 2 and 4 either way


def test_bit_63_of_a_64_camera_table(gpu):
    w, h = 32, 24
    frames2, Ks2, V2, u2, pos, R = vs.scene(7102, 2, w, h)
    F, KK = np.zeros((64, h, w), np.uint16), np.ascontiguousarray(np.broadcast_to(Ks2[0], (64, 3, 3)))
    VV, uu = np.ascontiguousarray(np.broadcast_to(np.eye(3, dtype=np.float32), (64, 3, 3))), np.zeros((64, 3), np.float32)
    for src, dst in ((0, 0), (1, 63)):
        F[dst], VV[dst], uu[dst] = frames2[src], V2[src], u2[src]
    start = world_start(7102, pos, R, 20.0, 10.0)
    prm = fit.fit_params(min_points=6)
    items = [(0, 0, 1 | 1 << 63) + start + (1.0,), (0, 0, 1 << 63) + start + (1.0,), (63, 0, 1) + start + (1.0,), (0, 0, 2 ** 64 - 1) + start + (1.0,)]
    out, rec = check(gpu, F, KK, VV, uu, instances(items), prm)
    assert rec["views_used"].tolist() == [1 | 1 << 63, 1 << 63, 1, 1 | 1 << 63] and (rec["points"] > 0).all()
    assert out[1].tobytes()[16:64] == out[2].tobytes()[16:64] and out[0].tobytes()[16:64] == out[3].tobytes()[16:64]


@pytest.mark.parametrize("model,points", [(1, 1), (2, 257), (3, 1024), (4, 1025)])
def test_model_sizes(gpu, model, points):
    ms, _ = gpu
    assert ms[model].info()[0] == points
    frames, Ks, V, u, pos, R = vs.scene(7103, 2, 96, 96)
    items = [(0, model, 0b11) + world_start(7103, pos, R, 40.0, 10.0) + (1.0,), (0, model, 0b10, R, pos, 1.0)]
    out, rec = check(gpu, frames, Ks, V, u, instances(items))
    if points == 1:
        assert (rec["status"] == fit.FIT_FEW_POINTS).all() and (rec["steps"] == 0).all() and (rec["points"] <= 2).all()
    else:
        assert (rec["status"] == fit.FIT_OK).all() and (rec["points"] > 60).all() and np.linalg.norm(out["t"][0] - pos) < 10.0


def test_the_term_limit_on_either_side(gpu):
    ms, ft = gpu
    yaws = (-70.0, -50.0, -30.0, -10.0, 10.0, 30.0, 50.0, 70.0)
    frames, Ks, V, u, pos, R = vs.scene(7104, 8, 64, 48, yaws=yaws)
    start = world_start(7104, pos, R, 20.0, 10.0)
    out, rec = check(gpu, frames, Ks, V, u, instances([(0, 5, 0xFF) + start + (1.0,)]))           # 8 x 4096 = DH_FIT_MAX_POINTS terms
    assert rec["status"][0] == fit.FIT_OK and rec["views_used"][0] == 0xFF
    with Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        with pytest.raises(_lib.DepthheadError) as ei:
            ft.fit_views(frames, ms, instances([(0, 6, 0xFF) + start + (1.0,)]), views)
        assert ei.value.code == -1 and "32776 terms" in str(ei.value)
        ft.fit_views(frames, ms, instances([(0, 6, 0x7F) + start + (1.0,)]), views)                 # 7 x 4097 pass


@functools.lru_cache(maxsize=None)
def two_rigs():
    """Seven cameras at 96 x 96: rig A cameras 0 - 2, rig B cameras 3 - 6 of which 5 and 6 are empty; four instances, the last
    sees only the empty cameras."""
    a, b = vs.scene(7105, 3, 96, 96), padded(7106, 2, 96, 96, 0, 2)
    frames, Ks, V, u = (np.concatenate([a[k], b[k]]) for k in range(4))
    items = [(0, 0, 0b111) + world_start(7105, a[4], a[5]) + (1.0,), (0, 0, 0b110) + world_start(7136, a[4], a[5], 20.0, 10.0) + (1.0,),
             (3, 0, 0b0111) + world_start(7106, b[4], b[5], 60.0, 20.0) + (1.0,), (3, 0, 0b1100) + world_start(7106, b[4], b[5], 20.0, 10.0) + (1.0,)]
    inst = instances(items)
    for x in (frames, Ks, V, u, inst):
        x.setflags(write=False)
    return frames, Ks, V, u, inst


@functools.lru_cache(maxsize=None)
def two_rigs_expected():
    out, rec = expected(*two_rigs())
    out.setflags(write=False); rec.setflags(write=False)
    return out, rec


def test_four_instances_over_two_rigs_in_one_launch(gpu):
    ms, ft = gpu
    frames, Ks, V, u, inst = two_rigs()
    with Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        a = ft.fit_views(frames, ms, inst, views)
        b = ft.fit_views(frames, ms, inst, views)
    want_out, want_rec = two_rigs_expected()
    same_records(a[1], want_rec, "record"); same_records(a[0], want_out, "instance")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()                   # two runs of one call
    assert a[1]["status"].tolist() == [fit.FIT_OK] * 3 + [fit.FIT_FEW_POINTS] and a[1]["views_used"].tolist() == [0b111, 0b110, 0b011, 0]
    assert a[0][3].tobytes() == inst[3].tobytes() and a[1]["points"][3] == 0


@pytest.mark.parametrize("coarse,full", [(0, 14), (6, 0), (0, 0), (32, 32)])
def test_schedules(gpu, coarse, full):
    frames, Ks, V, u, pos, R = vs.scene(7107, 2, 96, 96)
    inst = instances([(0, 0, 0b11) + world_start(7107, pos, R, 20.0, 10.0) + (1.0,)])
    out, rec = check(gpu, frames, Ks, V, u, inst, fit.fit_params(coarse_iterations=coarse, iterations=full))
    assert rec["steps"][0] <= coarse + full and rec["status"][0] == fit.FIT_OK
    if coarse + full == 0:
        assert out.tobytes() == inst.tobytes() and rec["points"][0] > 0 and rec["sum_r2_fixed"][0] > 0 and rec["views_used"][0] == 0b11


def test_lambda_0_and_1e8_and_both_early_exits(gpu):
    frames, Ks, V, u, pos, R = vs.scene(7003, 3)
    inst = instances([(0, 0, 0b111) + world_start(7003 + 31, pos, R, 20.0, 10.0) + (1.0,)])
    out, rec = check(gpu, frames, Ks, V, u, inst, fit.fit_params(lam=1e8))
    assert rec["steps"].tolist() == [2] and rec["status"].tolist() == [fit.FIT_OK]              # one coarse step, one full step
    out, rec = check(gpu, frames, Ks, V, u, inst, fit.fit_params(lam=1e7))
    assert rec["steps"].tolist() == [7]
    check(gpu, frames, Ks, V, u, inst, fit.fit_params(lam=0.0, gate=(200.0, 40.0)))


def test_min_points_on_either_side_of_the_summed_count(gpu):
    frames, Ks, V, u, pos, R = vs.scene(7000, 3)
    v, nm = host_models()[0]
    R0, t0 = world_start(7000 + 31, pos, R, 20.0, 10.0)
    Rd, td = R0.astype(np.float64), t0.astype(np.float64)
    each = [vr.one_pass(frames, Ks, V, u, c, 1, v, nm, 1.0, Rd, td, 120.0)[3] for c in range(3)]
    total = sum(each)
    assert max(each) < total
    inst = instances([(0, 0, 0b111, R0, t0, 1.0)])
    out, rec = check(gpu, frames, Ks, V, u, inst, fit.fit_params(coarse_iterations=1, iterations=0, min_points=total))
    assert (rec["status"][0], rec["steps"][0]) == (fit.FIT_OK, 1)
    out, rec = check(gpu, frames, Ks, V, u, inst, fit.fit_params(coarse_iterations=1, iterations=0, min_points=total + 1))
    assert (rec["status"][0], rec["steps"][0]) == (fit.FIT_FEW_POINTS, 0) and out.tobytes() == inst.tobytes()


def test_singular_exit_and_a_camera_that_is_no_pinhole(gpu):
    """Camera 1 of three has a K with skew and a third row that is not (0, 0, 1), and is rendered through it; then section
    18's plane before a wall in camera 2 with lambda = 0."""
    w, h = 96, 96
    _, Ks, V, u, pos, R = vs.scene(7108, 3, w, h)
    Ks = Ks.copy()
    Ks[1, 0, 0] *= 1.3; Ks[1, 0, 1] = 3.0; Ks[1, 2, 0] = 1e-4; Ks[1, 0, 2] += 5.5
    v, t, _ = fs.head()
    items = [rr.instance(f, m, Rc, tc, head=hd) for f, m, Rc, tc, _, hd in vs.view_items(pos, R, V, u)]
    frames, _ = rr.render([(v, t), fs.torso()], items, 3, w, h, Ks, noise=2, holes=0.02, seed=8)
    out, rec = check(gpu, frames, Ks, V, u, instances([(0, 0, 0b111) + world_start(7108, pos, R, 40.0, 15.0) + (1.0,), (1, 0, 0b1) + world_start(7108, pos, R, 40.0, 15.0) + (1.0,)]))
    assert (rec["status"] == fit.FIT_OK).all() and rec["views_used"].tolist() == [0b111, 1] and np.linalg.norm(out["t"][0] - pos) < 10.0
    wall = np.zeros((3, h, w), np.uint16)
    wall[2] = 800
    Vd, ud = V[2].astype(np.float64), u[2].astype(np.float64)
    Rc0, tc0 = render.euler_to_matrix((0, 4, 3)).astype(np.float64), np.array([0.0, 0.0, 810.0])
    inst = instances([(0, 7, 0b110, Vd.T @ Rc0, Vd.T @ (tc0 - ud), 1.0)])
    K0 = np.ascontiguousarray(np.broadcast_to(synth.default_intrinsic(w, h), (3, 3, 3)))
    out, rec = check(gpu, wall, K0, V, u, inst, fit.fit_params(coarse_iterations=0, iterations=3, lam=0.0))
    assert rec["status"][0] == fit.FIT_SINGULAR and rec["steps"][0] == 0 and rec["views_used"][0] == 0b100 and out.tobytes() == inst.tobytes()


def test_host_form_against_the_device_twin_chained_after_a_device_render(gpu):
    """dh_render_depth_cameras_device and dh_fit_depth_views_device on one side stream with no host copy or wait between them;
    the outputs lie between 4 KB guard bands at pointers 8 bytes off a 256-byte line."""
    import torch
    ms, ft = gpu
    w, h, n = 96, 96, 4
    _, Ks3, V3, u3, pos, R = vs.scene(7109, 3, w, h)
    Ks, V, u = np.concatenate([Ks3, Ks3[:1]]), np.concatenate([V3, V3[:1]]), np.concatenate([u3, u3[:1]])     # camera 3 sees nothing
    v, t, _ = fs.head()
    bv, bt = fs.torso()
    inst = instances([(0, 0, 0b111) + world_start(7109, pos, R, 60.0, 20.0) + (1.0,), (0, 0, 0b1010) + world_start(7109, pos, R, 20.0, 10.0) + (1.0,),
                      (3, 0, 0b1) + world_start(7109, pos, R, 20.0, 10.0) + (1.0,)])
    sizes = (len(inst) * INST.itemsize, len(inst) * REC.itemsize)
    stream = torch.cuda.Stream()
    with render.Mesh(v, t) as head, render.Mesh(bv, bt) as box, render.Renderer() as rd, Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        bufs = [torch.full((GUARD + 8 + s + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for s in sizes]
        handles = (C.c_void_p * len(ms))(*[m._h.value for m in ms])
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            frames, _ = rd.render([head, box], render.instances(vs.view_items(pos, R, V3, u3)), n, w, h, cams, noise=2, holes=0.02, seed=3,
                                  device_out=True, masks=False)
            _lib.check(ft._lib.dh_fit_depth_views_device(ft._h, C.c_void_p(frames.data_ptr()), w, h, views._h, handles, C.c_uint32(len(ms)),
                                                         _lib.vp(inst), C.c_uint32(len(inst)), None, C.c_void_p(bufs[0].data_ptr() + GUARD + 8),
                                                         C.c_void_p(bufs[1].data_ptr() + GUARD + 8), C.c_void_p(stream.cuda_stream)))
            d_out, d_rec = ft.fit_views(frames, ms, inst, views, device_out=True, stream=stream.cuda_stream)
        stream.synchronize()
        host = frames.cpu().view(torch.int16).numpy().view(np.uint16)
        h_out, h_rec = ft.fit_views(host, ms, inst, views)
    want_out, want_rec = expected(host, Ks, V, u, inst)
    same_records(h_rec, want_rec, "host record"); same_records(h_out, want_out, "host instance")
    for buf, size, dt, want in ((bufs[0], sizes[0], INST, want_out), (bufs[1], sizes[1], REC, want_rec)):
        raw = buf.cpu().numpy()
        assert (raw[:GUARD + 8] == 0xEE).all() and (raw[GUARD + 8 + size:] == 0xEE).all()
        same_records(raw[GUARD + 8:GUARD + 8 + size].copy().view(dt), want, "device form")
    same_records(d_out.cpu().numpy().view(INST), want_out, "device instance"); same_records(d_rec.cpu().numpy().view(REC), want_rec, "device record")
    assert h_rec["status"].tolist() == [fit.FIT_OK, fit.FIT_OK, fit.FIT_FEW_POINTS] and h_rec["views_used"].tolist() == [0b111, 0b0010, 0]
    assert np.linalg.norm(h_out["t"][0] - pos) < 10.0


def test_a_fitter_reused_with_a_smaller_a_larger_and_an_empty_call(gpu):
    ms, _ = gpu
    frame, K, pos, R = fs.scene(96, 96, 7100)
    single = np.zeros(1, _lib.RENDER_INSTANCE_DTYPE)
    R0, t0 = fs.start(7100, pos, R, 90.0, 25.0)
    single[0] = (0, 0, R0.reshape(9), t0, 1.0, 0)
    sf, sK, sV, su, spos, sR = vs.scene(7100, 2, 96, 96)
    small = instances([(0, 0, 0b11) + world_start(7100, spos, sR) + (1.0,)])
    want_small = expected(sf, sK, sV, su, small)
    frames, Ks, V, u, inst = two_rigs()
    with fit.Fitter() as ft, Cameras(sK) as c2, fit.Views(c2, sV, su) as v2, Cameras(Ks) as c7, fit.Views(c7, V, u) as v7:
        before = ft.fit(frame[None], ms, single, K)
        for _ in range(2):
            out, rec = ft.fit_views(sf, ms, small, v2)
            same_records(rec, want_small[1], "small record"); same_records(out, want_small[0], "small instance")
            out, rec = ft.fit_views(frames, ms, inst, v7)
            same_records(rec, two_rigs_expected()[1], "large record"); same_records(out, two_rigs_expected()[0], "large instance")
        out, rec = ft.fit_views(sf, ms, [], v2)
        assert len(out) == 0 and len(rec) == 0
        after = ft.fit(frame[None], ms, single, K)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()


def test_one_call_captured_in_a_graph_and_replayed_twice(gpu):
    """The eager call first (it uploads the fitter's tables), then the capture of the same call -- the kernel alone, nothing
    else is asked of the runtime while the stream captures -- then two replays, each equal to the restatement; a captured call
    whose tables are not the fitter's last is refused with DH_ESTATE."""
    import torch
    ms, ft = gpu
    frames, Ks, V, u, inst = two_rigs()
    want_out, want_rec = two_rigs_expected()
    with Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            out, rec = ft.fit_views(d_frames, ms, inst, views, device_out=True)
        stream.synchronize()
        same_records(rec.cpu().numpy().view(REC), want_rec, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, rec = ft.fit_views(d_frames, ms, inst, views, device_out=True)
            with pytest.raises(_lib.DepthheadError) as ei:
                ft.fit_views(d_frames, ms, inst[1:3], views, device_out=True)
            assert ei.value.code == -6 and "captured" in str(ei.value)
        for _ in range(2):
            out.fill_(0xEE); rec.fill_(0xEE)
            g.replay()
            torch.cuda.synchronize()
            same_records(rec.cpu().numpy().view(REC), want_rec, "replay record"); same_records(out.cpu().numpy().view(INST), want_out, "replay instance")
        del g


def test_refusals_that_need_a_device(gpu):
    ms, ft = gpu
    frames, Ks, V, u, pos, R = vs.scene(7100, 2, 96, 96)
    start = world_start(7100, pos, R)

    def refused(what, fn):
        with pytest.raises(_lib.DepthheadError) as ei:
            fn()
        assert ei.value.code == -1 and what in str(ei.value), str(ei.value)

    with Cameras(Ks) as cams:
        for idx, x, what in ((0, np.nan, "view 1 has a non-finite"), (4, np.inf, "view 1 has a non-finite"), (0, V[1, 0, 0] + 0.002, "(V V^T)[0][0]"),
                             (5, V[1, 1, 2] + 0.002, "(V V^T)[1][2]")):
            bad = V.copy()
            bad.reshape(2, 9)[1, idx] = x
            refused(what, lambda: fit.Views(cams, bad, u))
        bad = u.copy()
        bad[0, 2] = -np.inf
        refused("view 0 has a non-finite", lambda: fit.Views(cams, V, bad))
        ok = V.copy()
        ok[1, 0, 0] += 0.0002                                           # within DH_FIT_VIEW_TOLERANCE
        fit.Views(cams, ok, u).close()
        with fit.Views(cams, V, u) as views:
            def call(items, fr_=frames, prm=None):
                return lambda: ft.fit_views(fr_, ms, instances(items), views, params=prm)
            refused("seen by no view", call([(0, 0, 0) + start + (1.0,)]))
            refused("names camera 2 of 2", call([(0, 0, 0b100) + start + (1.0,)]))
            refused("names camera 2 of 2", call([(1, 0, 0b11) + start + (1.0,)]))
            refused("names camera 4294967295 of 2", call([(0xFFFFFFFF, 0, 1) + start + (1.0,)]))
            refused("names camera 4294967358 of 2", call([(0xFFFFFFFF, 0, 1 << 63) + start + (1.0,)]))
            refused("names model 8 of 8", call([(0, 8, 1) + start + (1.0,)]))
            refused("non-finite R, t or scale", call([(0, 0, 1, start[0], (0.0, np.nan, 900.0), 1.0)]))
            refused("not orthonormal: (R R^T)[0][0]", call([(0, 0, 1, np.diag([1.011, 1.0, 1.0]), start[1], 1.0)]))
            radius = ms[0].info()[1]
            refused("mm from its origin", call([(0, 0, 1) + start + (float(np.float32(4096.5 / radius)),)]))
            refused("min_points 5 below 6", call([(0, 0, 1) + start + (1.0,)], prm=fit.fit_params(min_points=5)))
            refused("gate[1]", call([(0, 0, 1) + start + (1.0,)], prm=fit.fit_params(gate=(120.0, 0.0))))
            assert ft._lib.dh_fit_depth_views(ft._h, _lib.vp(frames), 0, 96, views._h, None, 0, None, 0, None, _lib.vp(np.zeros(72, np.uint8)),
                                              _lib.vp(np.zeros(32, np.uint8))) == -1 and "frame size" in ft._lib.dh_last_error().decode()
            with pytest.raises(ValueError):
                ft.fit_views(frames[:1], ms, instances([(0, 0, 1) + start + (1.0,)]), views)


def test_view_instances_from_persons_on_a_two_camera_rig_tracker_step(gpu):
    """Three cameras in two rigs: camera 0 alone, cameras 1 and 2 the rig of two, so that the rig's first camera is not camera
    0.  Every camera sees the same frame; camera 2 is turned 20 degrees about y and placed so that its heaviest head
    lies on camera 1's in the world, and the two views fuse into one person.  The helper is outside the bit-exact contract:
    its instances are held to the step's records field by field, and the fit of them to the restatement as every call is."""
    from depthhead_amd import prediction, tracking
    w, h = 128, 112
    rig_begin = [0, 1, 3]
    frames = np.ascontiguousarray(np.broadcast_to(synth.biwi_batch(1, w, h, first=4), (3, h, w)))
    Ks = np.ascontiguousarray(np.broadcast_to(synth.default_intrinsic(w, h), (3, 3, 3)))
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)
    rig_R = np.stack([np.eye(3), np.eye(3), render.euler_to_matrix((0, 20, 0)).astype(np.float64)]).astype(np.float32)
    rig_t = np.zeros((3, 3), np.float32)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, Cameras(Ks) as cams:
        n0, heads0 = hp.predict_heads_cameras(frames, cams, 4, 30)
        assert n0[1] > 0 and n0[0] == n0[2] == n0[1], n0
        m = heads0[1, 0]["pose"]["mid_point"].astype(np.float64)
        rig_t[2] = m - rig_R[2].astype(np.float64) @ m
        with tracking.Rig(cams, rig_R, rig_t, rig_begin) as rig, tracking.RigTracker(hp, rig, w, h) as tr:
            n_heads, heads, _, n_persons, persons, _ = tr.step(frames)
    assert heads.shape == (3, tr.max_heads) and persons.shape == (2, _lib.RIG_MAX_PERSONS)
    assert np.array_equal(n_heads, n0) and (n_persons >= 1).all(), (n_heads, n_persons)
    both = 0
    per_rig = []
    for g in range(2):
        a, b = rig_begin[g], rig_begin[g + 1]
        ps = persons[g][:n_persons[g]]
        inst = fit.view_instances_from_persons(ps, heads, rig_R, rig_t, a, scale=0.95, model=0)
        assert inst.dtype == INST and inst.shape == (n_persons[g],)
        for p, it in zip(ps, inst):
            cam, hd = int(p["best_cam"]), int(p["best_head"])
            assert a <= cam < b and hd < n_heads[cam]                                       # an index into the whole camera table
            assert it["first_cam"] == a and it["views"] == p["views"] != 0 and int(p["views"]) >> (b - a) == 0
            assert int(p["views"]) >> (cam - a) & 1 and bin(int(p["views"])).count("1") == p["n_views"]
            assert it["t"].tobytes() == p["world"].tobytes() and it["scale"] == np.float32(0.95) and it["model"] == 0 and it["flags"] == 0
            Rw = tracking.world_rotation(rig_R[cam], heads[cam, hd]["pose"]["rotation"])
            assert it["R"].tobytes() == Rw.astype(np.float32).tobytes()
            R64 = it["R"].reshape(3, 3).astype(np.float64)
            assert np.abs(R64 @ R64.T - np.eye(3)).max() < 1e-5 and np.linalg.det(R64) > 0.0
            both += p["views"] == 0b11
        per_rig.append(inst)
    assert both >= 1                                                                        # the rig's two views of one head fused
    V, u = fit.views_from_rig(rig_R, rig_t)
    inst = np.concatenate(per_rig)
    out, rec = check(gpu, frames, Ks, V, u, inst)
    assert np.isin(rec["status"], (fit.FIT_OK, fit.FIT_FEW_POINTS, fit.FIT_SINGULAR)).all()
    assert (rec["views_used"] & ~inst["views"] == 0).all() and (out["views"] == inst["views"]).all() and (out["first_cam"] == inst["first_cam"]).all()
    seen = rec["points"] > 0
    assert seen.any() and (rec["views_used"][seen] != 0).all()
