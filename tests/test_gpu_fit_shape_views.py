"""The multi-view shape step on the GPU (k_fit_shape_views.hip) against its restatement
tests/shape_views_ref.py: every byte of every dh_shape_record equal, with no tolerance.  Scenes are those of
tests/shape_views_scenes.py (the stretched subject seen by three cameras on an arc at several sets); what is compared is the
arithmetic, so the instances are true or rough world poses wherever a fitted one is not what the test is about."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import shape_ref as sr
import shape_scenes as ss
import shape_views_ref as svr
import shape_views_scenes as sv
import view_fit_ref as vr
from gpu_kit import fit_models, same_records
from depthhead_amd import _lib, fit, synth
from depthhead_amd.tracking import Cameras

pytestmark = pytest.mark.gpu

INST, REC = _lib.VIEW_INSTANCE_DTYPE, _lib.SHAPE_RECORD_DTYPE
GUARD = 4096
SKIP = svr.SKIP


def fields8(v, n):
    """Eight fields of a model: head_basis's four, three shears and 10 mm along the normal."""
    v = np.asarray(v, np.float64)
    z = np.zeros(len(v))
    extra = [np.stack([v[:, 1], z, z], 1), np.stack([z, v[:, 2], z], 1), np.stack([z, z, v[:, 0]], 1), 10.0 * np.asarray(n, np.float64)]
    return np.concatenate([synth.head_basis(v), np.array(extra, np.float32)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_models():
    """points -> (pts, nrm, fields [8, points, 3]): head_mesh(2) whole (162), head_mesh(4) whole (2562) and its first 64, 255, 256
    and 257 points -- a wave, either side of the workgroup's 256 lanes -- and one point that faces the yaw-0 camera."""
    v2, _, n2 = fs.head(2)
    v4, _, n4 = fs.head(4)
    B2, B4 = fields8(v2, n2), fields8(v4, n4)
    front = int(np.argmin(v2[:, 2]))
    out = {162: (v2, n2, B2), 2562: (v4, n4, B4), 1: (v2[front:front + 1].copy(), n2[front:front + 1].copy(), B2[:, front:front + 1].copy())}
    for k in (64, 255, 256, 257):
        out[k] = (v4[:k].copy(), n4[:k].copy(), B4[:, :k].copy())
    return out


@pytest.fixture(scope="module")
def gpu():
    with fit_models(host_models()) as both:
        yield both


@contextlib.contextmanager
def rig(Ks, V, u):
    with Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        yield views


def ref_params(prm):
    return svr.params() if prm is None else svr.params(prm.gate, prm.lam, prm.min_points)


def same(got, want, what):
    assert got.dtype == REC
    same_records(got, want, what)


def check(gpu, scene, points, nk, inst, sets=None, subjects=None, ns=1, prm=None):
    """One host call on model `points` with its first nk fields, against the restatement.  scene: (frames, Ks, V, u, ...)."""
    ms, ft = gpu
    frames, Ks, V, u = scene[:4]
    pts, nrm, B = host_models()[points]
    with fit.ShapeBasis(B[:nk]) as sb, rig(Ks, V, u) as views:
        got = ft.shape_step_views(frames, views, ms[points], sb, inst, sets=sets, subjects=subjects, n_subjects=ns, params=prm)
    want = svr.shape_step(frames, Ks, V, u, pts, nrm, B[:nk], inst, sets, subjects, ns, ref_params(prm))
    same(got, want, "record")
    return got


@functools.lru_cache(maxsize=None)
def subject_instances(seed=0, n_sets=2, w=160, h=120):
    """(scene, instances [2 * n_sets], sets): the subject's true world poses, then its rough starts, all three views each."""
    scene = sv.subject(seed, n_sets, w, h)
    pos, Rs = scene[4], scene[5]
    inst = sv.as_records(sv.true_instances(pos, Rs) + sv.rough_instances(seed, pos, Rs))
    inst["flags"] = 0x5A0000 + np.arange(len(inst))      # ignored by the step
    inst["model"][1::2] = 7                              # ignored too: a call has one model
    inst.setflags(write=False)
    sets = np.tile(np.arange(n_sets, dtype=np.uint32), 2)
    sets.setflags(write=False)
    return scene, inst, sets


def test_one_instance_one_identity_view_one_field_is_also_the_single_view_step(gpu):
    ms, ft = gpu
    frame, K, pos, R = fs.scene(96, 96, 7100)
    eye, zero = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)
    world = sv.as_records([{"first_cam": 0, "views": 1, "R": R, "t": pos, "scale": 1.0}])
    prm = fit.shape_params(min_points=16)
    rec = check(gpu, (frame[None, None], K[None], eye, zero), 162, 1, world, prm=prm)
    assert rec["status"][0] == fit.SHAPE_OK and rec["points"][0] >= 30 and rec["instances"][0] == 1
    single = ss.as_records([{"frame": 0, "R": R, "t": pos, "scale": 1.0}])
    with fit.ShapeBasis(host_models()[162][2][:1]) as sb, Cameras(K[None]) as cams:
        same(ft.shape_step(frame[None], ms[162], sb, single, cams, params=prm), rec, "dh_fit_shape_cameras")
        same(ft.shape_step(frame[None], ms[162], sb, single, K, params=prm), rec, "dh_fit_shape")


@pytest.mark.parametrize("nk", range(1, 9))
def test_field_counts_with_three_views(gpu, nk):
    scene, inst, sets = subject_instances(0, 2, 96, 96)
    rec = check(gpu, scene, 162, nk, inst[:2], sets[:2])
    assert rec["status"][0] == fit.SHAPE_OK and rec["instances"][0] == 6 and (rec["delta"][0, :nk] != 0.0).all() and (rec["delta"][0, nk:] == 0.0).all()


@pytest.mark.parametrize("points", (1, 255, 256, 257, 2562))
def test_model_sizes(gpu, points):
    scene, inst, sets = subject_instances()
    rec = check(gpu, scene, points, 4, inst, sets, prm=fit.shape_params(min_points=1))
    assert rec["points"][0] > 0 and rec["status"][0] in (fit.SHAPE_OK, fit.SHAPE_SINGULAR)
    if points == 2562:
        assert rec["status"][0] == fit.SHAPE_OK and rec["points"][0] > 12 * 500 and rec["instances"][0] == 12


@functools.lru_cache(maxsize=None)
def wide_rig(n, w=96, h=96):
    """A table of n cameras: the three of the subject's rig over and over (camera c is camera c mod 3, with its frame)."""
    frames, Ks, V, u, pos, Rs = sv.subject(3, 1, w, h)
    pick = np.arange(n) % 3
    return sv.vs._ro(np.ascontiguousarray(frames[:, pick]), np.ascontiguousarray(Ks[pick]), np.ascontiguousarray(V[pick]),
                     np.ascontiguousarray(u[pick]), pos, Rs)


def world(scene, first_cam, views, s=0):
    return {"first_cam": first_cam, "views": views, "R": np.float32(scene[5][s]), "t": np.float32(scene[4][s]), "scale": np.float32(1.0)}


def test_masks_with_gaps_and_a_single_high_bit(gpu):
    scene = wide_rig(9)
    items = [world(scene, 0, 0b101), world(scene, 3, 1 << 5), world(scene, 2, 0b1010001), world(scene, 8, 1)]
    rec = check(gpu, scene, 162, 4, sv.as_records(items), subjects=np.arange(4, dtype=np.uint32), ns=4, prm=fit.shape_params(min_points=16))
    assert rec["instances"].tolist() == [2, 1, 3, 1] and (rec["status"] == fit.SHAPE_OK).all()


@pytest.mark.parametrize("n, first_cam", ((64, 0), (70, 6)))
def test_all_64_bits(gpu, n, first_cam):
    """64 views of one instance: every rank of the grid is busy; in a table of 70 cameras the ranks are fewer than the cameras."""
    scene = wide_rig(n)
    mask = (1 << 64) - 1
    rec = check(gpu, scene, 64, 4, sv.as_records([world(scene, first_cam, mask), world(scene, first_cam, 0b11)]), prm=fit.shape_params(min_points=1))
    assert rec["instances"][0] > 40 and rec["points"][0] > 0


def test_a_table_of_one_camera(gpu):
    scene = wide_rig(1)
    rec = check(gpu, scene, 162, 4, sv.as_records([world(scene, 0, 1), world(scene, 0, 1)]), prm=fit.shape_params(min_points=16))
    assert rec["instances"][0] == 2 and rec["status"][0] == fit.SHAPE_OK


def test_three_sets_in_mixed_order_and_no_sets(gpu):
    scene, inst, _ = subject_instances(1, 3)
    mixed = np.array([2, 0, 1, 1, 2, 0], np.uint32)
    six = inst[[2, 0, 1, 4, 5, 3]]
    rec = check(gpu, scene, 162, 4, six, mixed)
    assert rec["instances"][0] == 18 and rec["status"][0] == fit.SHAPE_OK
    same(check(gpu, scene, 162, 4, six[::-1].copy(), mixed[::-1].copy()), rec, "the order of the instances is free")
    first = check(gpu, scene, 162, 4, inst[[0, 3]])                   # sets = None: set 0
    same(check(gpu, scene, 162, 4, inst[[0, 3]], np.zeros(2, np.uint32)), first, "sets = None is set 0")
    same(check(gpu, (scene[0][:1],) + scene[1:], 162, 4, inst[[0, 3]]), first, "and the frames of one set alone")


def test_twelve_instances_in_three_subjects_with_an_empty_view_and_two_skipped(gpu):
    scene, inst, sets = subject_instances(0, 3)
    frames = scene[0].copy()
    frames[1, 2] = 0                                                  # camera 2 sees nothing at set 1
    scene = (frames,) + scene[1:]
    twelve = inst[np.arange(12) % 6].copy()
    twelve["t"][6:, 0] += np.float32(3.0)
    st = sets[np.arange(12) % 6]
    subjects = np.array([0, 0, 2, SKIP, 2, 2, 0, 0, SKIP, 2, 0, 2], np.uint32)
    rec = check(gpu, scene, 162, 4, twelve, st, subjects, 3)
    # instances 1, 4, 7 and 10 are in set 1, two pairs each: three of them in subject 0, one in subject 2
    assert rec["status"].tolist() == [fit.SHAPE_OK, fit.SHAPE_FEW_POINTS, fit.SHAPE_OK]
    assert rec["instances"].tolist() == [5 * 3 - 3, 0, 5 * 3 - 1] and rec["points"][1] == 0 and (rec["delta"][1] == 0.0).all()
    keep = subjects != SKIP
    same(check(gpu, scene, 162, 4, twelve[keep], st[keep], subjects[keep], 3), rec, "without the skipped")
    junk = twelve.copy()
    junk["t"][3] = (1e30, np.nan, 0.0); junk["first_cam"][8] = 4000; junk["R"][8] = np.inf; junk["views"][3] = 0
    ms, ft = gpu
    with fit.ShapeBasis(host_models()[162][2][:4]) as sb, rig(*scene[1:4]) as views:
        same(ft.shape_step_views(frames, views, ms[162], sb, junk, sets=st, subjects=subjects, n_subjects=3), rec, "junk in the skipped")
        for sj in (0, 2):                                             # two subjects in one call are two calls
            one = ft.shape_step_views(frames, views, ms[162], sb, twelve[subjects == sj], sets=st[subjects == sj])
            assert one[0].tobytes() == rec[sj].tobytes()


@functools.lru_cache(maxsize=None)
def many(count):
    """`count` (instance, view) pairs as single-view instances of the subject's three cameras at two sets, each true pose
    moved by a few seeded millimetres."""
    scene, inst, sets = subject_instances()
    out = inst[np.arange(count) % 2].copy()
    out["views"] = np.uint64(1) << (np.arange(count) // 2 % 3).astype(np.uint64)
    out["t"] += (6.0 * synth.SplitMix(4243).uniform(3 * count).reshape(count, 3) - 3.0).astype(np.float32)
    out.setflags(write=False)
    return scene, out, np.ascontiguousarray(sets[np.arange(count) % 2])


@pytest.mark.parametrize("count", (1, 255, 257))
def test_pair_counts_into_one_subject(gpu, count):
    scene, inst, sets = many(count)
    rec = check(gpu, scene, 162, 4, inst, sets, prm=fit.shape_params(min_points=16))
    assert rec["status"][0] == fit.SHAPE_OK and rec["instances"][0] == count and rec["points"][0] > 30 * count


def test_gates_and_min_points(gpu):
    scene, inst, sets = subject_instances()
    narrow = check(gpu, scene, 162, 4, inst, sets, prm=fit.shape_params(gate=1.0, min_points=1))
    wide = check(gpu, scene, 162, 4, inst, sets, prm=fit.shape_params(gate=256.0))
    usual = check(gpu, scene, 162, 4, inst, sets)
    assert 0 < narrow["points"][0] < usual["points"][0] < wide["points"][0]
    count = int(usual["points"][0])
    at = check(gpu, scene, 162, 4, inst, sets, prm=fit.shape_params(min_points=count))
    above = check(gpu, scene, 162, 4, inst, sets, prm=fit.shape_params(min_points=count + 1))
    assert at.tobytes() == usual.tobytes()
    assert above["status"][0] == fit.SHAPE_FEW_POINTS and (above["delta"] == 0.0).all()
    assert (above["points"][0], above["instances"][0], above["sum_r2_fixed"][0]) == (count, 12, usual["sum_r2_fixed"][0])


def test_both_exits(gpu):
    """FEW_POINTS: empty frames.  SINGULAR: two identical fields with lambda = 0 over 257 pairs, where the diagonal has grown
    past 2^53 * 1e-9 so that a + 1e-9 == a and the second pivot is a - (a / a) * a = 0 (section 20's case); over 6 pairs the
    same basis goes on by the 1e-9 term."""
    ms, ft = gpu
    scene, inst, sets = many(257)
    frames, Ks, V, u = scene[:4]
    pts, nrm, B = host_models()[162]
    twin = np.stack([B[0], B[0]])
    prm = fit.shape_params(lam=0.0)
    with fit.ShapeBasis(twin) as sb, rig(Ks, V, u) as views:
        empty = ft.shape_step_views(np.zeros_like(frames), views, ms[162], sb, inst, sets=sets, params=prm)
        same(empty, svr.shape_step(np.zeros_like(frames), Ks, V, u, pts, nrm, twin, inst, sets, prm=ref_params(prm)), "empty")
        assert (empty["status"][0], empty["points"][0], empty["instances"][0], empty["sum_r2_fixed"][0]) == (fit.SHAPE_FEW_POINTS, 0, 0, 0)
        got = ft.shape_step_views(frames, views, ms[162], sb, inst, sets=sets, params=prm)
        same(got, svr.shape_step(frames, Ks, V, u, pts, nrm, twin, inst, sets, prm=ref_params(prm)), "twin fields, 257 pairs")
        assert got["status"][0] == fit.SHAPE_SINGULAR and (got["delta"] == 0.0).all() and got["points"][0] > 0
        few = ft.shape_step_views(frames, views, ms[162], sb, inst[:6], sets=sets[:6], params=prm)
        same(few, svr.shape_step(frames, Ks, V, u, pts, nrm, twin, inst[:6], sets[:6], prm=ref_params(prm)), "twin fields, 6 pairs")
        assert few["status"][0] == fit.SHAPE_OK


def device_step(ft, views, model, sb, d_frames, inst, sets, subjects, ns, prm=None, stream=None):
    """The _device form on host arrays copied to the device; the records back on the host."""
    import torch
    d_inst = torch.from_numpy(np.ascontiguousarray(inst).view(np.uint8).copy()).cuda()
    d_sets = None if sets is None else torch.from_numpy(np.ascontiguousarray(sets, np.uint32).view(np.int32).copy()).cuda()
    d_subj = None if subjects is None else torch.from_numpy(np.ascontiguousarray(subjects, np.uint32).view(np.int32).copy()).cuda()
    rec = ft.shape_step_views(d_frames, views, model, sb, d_inst, sets=d_sets, subjects=d_subj, n_subjects=ns, params=prm, device_out=True, stream=stream)
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(REC)


BAD = ("no view", "a bit beyond n", "a set beyond n_sets", "a NaN in R", "a subject beyond n_subjects")


@pytest.mark.parametrize("which", range(len(BAD)))
def test_the_device_skips_an_instance_the_host_form_refuses(gpu, which):
    """One bad instance among good neighbours: the device leaves it out as a whole, the neighbours' records do not move, and the
    host form refuses the call."""
    import torch
    ms, ft = gpu
    scene, inst, sets = subject_instances()
    frames, Ks, V, u = scene[:4]
    pts, nrm, B = host_models()[162]
    bad, st = inst.copy(), sets.copy()
    subjects = np.array([0, 1, 0, 1], np.uint32)
    refusal = ["is seen by no view", "names camera 3 of 3", "names set 2 of 2", "has a non-finite R, t or scale", "names subject 2 of 2"][which]
    if which == 0:
        bad["views"][1] = 0
    elif which == 1:
        bad["views"][1] = 0b1011
    elif which == 2:
        st[1] = 2
    elif which == 3:
        bad["R"][1, 5] = np.nan
    else:
        subjects[1] = 2
    with fit.ShapeBasis(B[:4]) as sb, rig(Ks, V, u) as views:
        with pytest.raises(_lib.DepthheadError) as ei:
            ft.shape_step_views(frames, views, ms[162], sb, bad, sets=st, subjects=subjects, n_subjects=2)
        assert ei.value.code == -1 and "instance 1 " + refusal in str(ei.value), str(ei.value)
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        got = device_step(ft, views, ms[162], sb, d_frames, bad, st, subjects, 2)
        good = device_step(ft, views, ms[162], sb, d_frames, inst, sets, np.array([0, 1, 0, 1], np.uint32), 2)
    without = np.array([0, SKIP, 0, 1], np.uint32)
    same(got, svr.shape_step(frames, Ks, V, u, pts, nrm, B[:4], inst, sets, without, 2), BAD[which])
    same(got, svr.shape_step(frames, Ks, V, u, pts, nrm, B[:4], bad, st, subjects, 2), "the restated skip")
    assert got[0].tobytes() == good[0].tobytes() and got["instances"].tolist() == [6, 3] and good["instances"].tolist() == [6, 6]


def test_device_twin_chained_after_a_device_fit(gpu):
    """dh_fit_depth_views_device, then dh_fit_shape_views_device on its `out`, on a side stream with no host copy or wait between
    them; the records lie between 4 KB guard bands at a pointer that is 8 bytes off a 256-byte line."""
    import torch
    ms, ft = gpu
    scene = sv.subject(2, 1)
    frames, Ks, V, u, pos, Rs = scene
    pts, nrm, B = host_models()[162]
    starts = sv.as_records(sv.rough_instances(2, pos, Rs) + sv.rough_instances(3, pos, Rs, 10.0, 4.0) + sv.rough_instances(4, pos, Rs, 20.0, 5.0))
    starts["views"] = (0b111, 0b011, 0b110)
    subjects = np.array([0, 1, 0], np.uint32)
    ns, bytes_ = 2, 2 * REC.itemsize
    stream = torch.cuda.Stream()
    with fit.ShapeBasis(B[:4]) as sb, rig(Ks, V, u) as views:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_subj = torch.from_numpy(subjects.view(np.int32).copy()).cuda()
        buf = torch.full((GUARD + 8 + bytes_ + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            d_out, d_rec = ft.fit_views(d_frames[0], [ms[162]], starts, views, device_out=True, stream=stream.cuda_stream)
            _lib.check(ft._lib.dh_fit_shape_views_device(
                ft._h, C.c_void_p(d_frames.data_ptr()), C.c_uint32(1), 160, 120, views._h, ms[162]._h, sb._h, C.c_void_p(d_out.data_ptr()),
                C.c_uint32(3), None, C.c_void_p(d_subj.data_ptr()), C.c_uint32(ns), None, C.c_void_p(buf.data_ptr() + GUARD + 8),
                C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        fitted = d_out.cpu().numpy().view(INST)
        status = d_rec.cpu().numpy().view(_lib.VIEW_FIT_RECORD_DTYPE)["status"]
        host = ft.shape_step_views(frames, views, ms[162], sb, fitted, subjects=subjects, n_subjects=ns)
    want = svr.shape_step(frames, Ks, V, u, pts, nrm, B[:4], fitted, None, subjects, ns)
    same(host, want, "host form on the fitted instances")
    raw = buf.cpu().numpy()
    assert (raw[:GUARD + 8] == 0xEE).all() and (raw[GUARD + 8 + bytes_:] == 0xEE).all()
    same(raw[GUARD + 8:GUARD + 8 + bytes_].copy().view(REC), want, "device form")
    assert (status == fit.FIT_OK).all() and want["status"].tolist() == [fit.SHAPE_OK, fit.SHAPE_OK] and want["instances"].tolist() == [5, 2]


def test_a_fitter_reused_and_the_other_calls_unchanged(gpu):
    """A smaller, a larger and an empty call, twice over; Fitter.shape_step and Fitter.fit_views give the same bytes before and
    after, and one call run twice the same bytes."""
    ms, _ = gpu
    scene, inst, sets = subject_instances(0, 3)
    frames, Ks, V, u = scene[:4]
    pts, nrm, B = host_models()[162]
    small_scene = wide_rig(1)
    small = sv.as_records([world(small_scene, 0, 1)])
    prm = fit.shape_params(min_points=16)
    want_small = svr.shape_step(*small_scene[:4], pts, nrm, B[:4], small, prm=ref_params(prm))
    want_large = svr.shape_step(frames, Ks, V, u, pts, nrm, B[:4], inst, sets, np.arange(6, dtype=np.uint32) % 3, 3, ref_params(prm))
    single = ss.as_records([dict(s, frame=0) for s in sv.single_view(sv.true_instances(scene[4], scene[5])[:1], V, u)])
    starts = inst[3:4].copy()
    starts["model"] = 0
    with fit.Fitter() as ft, fit.ShapeBasis(B[:4]) as sb, rig(Ks, V, u) as views, rig(*small_scene[1:4]) as small_views:
        before = ft.fit_views(frames[0], [ms[162]], starts, views)
        before_shape = ft.shape_step(frames[0, 1:2], ms[162], sb, single, Ks[1], params=prm)
        for _ in range(2):
            same(ft.shape_step_views(small_scene[0], small_views, ms[162], sb, small, params=prm), want_small, "small")
            same(ft.shape_step_views(frames, views, ms[162], sb, inst, sets=sets, subjects=np.arange(6) % 3, n_subjects=3, params=prm), want_large,
                 "large")
        none = ft.shape_step_views(frames, views, ms[162], sb, inst[:0], n_subjects=2)
        assert none["status"].tolist() == [fit.SHAPE_FEW_POINTS] * 2 and not none["points"].any() and not none["delta"].any()
        same(none, svr.shape_step(frames, Ks, V, u, pts, nrm, B[:4], inst[:0], n_subjects=2), "empty call")
        after = ft.fit_views(frames[0], [ms[162]], starts, views)
        after_shape = ft.shape_step(frames[0, 1:2], ms[162], sb, single, Ks[1], params=prm)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert before_shape.tobytes() == after_shape.tobytes() and before_shape["points"][0] > 16


def graph_shape(lib, graph):
    """(node types, edges as index pairs) of a captured graph, asked of the HIP runtime the library is linked to."""
    n = C.c_size_t(0)
    assert lib.hipGraphGetNodes(C.c_void_p(graph), None, C.byref(n)) == 0
    nodes = (C.c_void_p * n.value)()
    assert lib.hipGraphGetNodes(C.c_void_p(graph), nodes, C.byref(n)) == 0
    types = []
    for node in nodes:
        t = C.c_int(-1)
        assert lib.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == 0
        types.append(t.value)
    e = C.c_size_t(0)
    assert lib.hipGraphGetEdges(C.c_void_p(graph), None, None, C.byref(e)) == 0
    src, dst = (C.c_void_p * max(e.value, 1))(), (C.c_void_p * max(e.value, 1))()
    if e.value:
        assert lib.hipGraphGetEdges(C.c_void_p(graph), src, dst, C.byref(e)) == 0
    where = {node: i for i, node in enumerate(nodes)}
    return types, [(where[src[i]], where[dst[i]]) for i in range(e.value)]


def test_one_call_captured_in_a_graph_and_replayed_twice(gpu):
    """The eager call first (it takes the fitter's sums buffer), then the capture, then two replays, each equal to the
    restatement.  The captured graph holds three kernel nodes in a chain: clear, accumulate, solve."""
    import torch
    ms, ft = gpu
    scene, inst, sets = subject_instances()
    frames, Ks, V, u = scene[:4]
    pts, nrm, B = host_models()[162]
    subjects = np.arange(4, dtype=np.uint32) % 2
    want = svr.shape_step(frames, Ks, V, u, pts, nrm, B[:4], inst, sets, subjects, 2)
    with fit.ShapeBasis(B[:4]) as sb, rig(Ks, V, u) as views:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_inst = torch.from_numpy(inst.view(np.uint8).copy()).cuda()
        d_sets = torch.from_numpy(sets.view(np.int32).copy()).cuda()
        d_subj = torch.from_numpy(subjects.view(np.int32).copy()).cuda()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            eager = ft.shape_step_views(d_frames, views, ms[162], sb, d_inst, sets=d_sets, subjects=d_subj, n_subjects=2, device_out=True)
        stream.synchronize()
        same(eager.cpu().numpy().view(REC), want, "eager")
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            rec = ft.shape_step_views(d_frames, views, ms[162], sb, d_inst, sets=d_sets, subjects=d_subj, n_subjects=2, device_out=True)
        types, edges = graph_shape(ft._lib, g.raw_cuda_graph())
        assert types == [0, 0, 0], types                               # hipGraphNodeTypeKernel
        assert sorted(len({a, b}) for a, b in edges) == [2, 2] and len({a for a, _ in edges}) == 2 and len({b for _, b in edges}) == 2
        assert len({a for a, _ in edges} & {b for _, b in edges}) == 1   # one node in the middle: a chain
        for _ in range(2):
            rec.fill_(0xEE)
            g.replay()
            torch.cuda.synchronize()
            same(rec.cpu().numpy().view(REC), want, "replay")


def test_two_runs_are_byte_identical(gpu):
    scene, inst, sets = many(255)
    a = check(gpu, scene, 162, 8, inst, sets, np.arange(255, dtype=np.uint32) % 5, 5)
    b = check(gpu, scene, 162, 8, inst, sets, np.arange(255, dtype=np.uint32) % 5, 5)
    assert a.tobytes() == b.tobytes() and (a["status"] == fit.SHAPE_OK).all()


def test_adapt_views_is_the_restated_adapt_views(gpu):
    """fit.adapt_views, two rounds over two sets, against shape_views_ref.adapt_views: the coefficients and the fitted instances
    to the bit."""
    _, ft = gpu
    v, t, _, B = ss.generic()
    frames, Ks, V, u, pos, Rs = sv.subject(12, 2)
    starts = sv.rough_instances(12, pos, Rs)
    with rig(Ks, V, u) as views:
        c, inst, trace = fit.adapt_views(ft, frames, views, v, t, B, sv.as_records(starts), sets=[0, 1], rounds=2)
    want_c, want_inst, want_trace = svr.adapt_views(frames, Ks, V, u, v, t, B, starts, [0, 1], fit.vertex_normals, rounds=2)
    assert c.tobytes() == want_c.tobytes() and len(trace) == 2
    assert inst.tobytes() == sv.as_records(want_inst).tobytes()
    for got, (wc, wfit, wrec) in zip(trace, want_trace):
        assert got["coeffs"].tobytes() == wc.tobytes() and got["shape"].tobytes() == wrec.tobytes()
        assert got["fit"]["points"].tolist() == [r["points"] for r in wfit] and got["fit"]["views_used"].tolist() == [r["views_used"] for r in wfit]
    assert (np.sign(c[:3]) == np.sign(sv.C_TRUE[:3])).all()


def test_refusals_that_need_a_model(gpu):
    import torch
    ms, ft = gpu
    scene, inst, sets = subject_instances()
    frames, Ks, V, u = scene[:4]
    pts, nrm, B = host_models()[162]

    def refused(what, fn):
        with pytest.raises(_lib.DepthheadError) as ei:
            fn()
        assert ei.value.code == -1 and what in str(ei.value) and "dh_fit_shape_views" in str(ei.value), str(ei.value)

    with fit.ShapeBasis(B[:4]) as sb, fit.ShapeBasis(host_models()[2562][2][:2]) as big, rig(Ks, V, u) as views:
        largest = sb.info()[2]
        radius = ms[162].info()[1]
        refused("the basis is one of 2562 points, the model has 162", lambda: ft.shape_step_views(frames, views, ms[162], big, inst, sets=sets))
        over = inst[:1].copy()
        for scale in (float(np.float32(256.5 / largest)), -float(np.float32(256.5 / largest))):
            over["scale"] = scale
            refused("scales the basis to", lambda: ft.shape_step_views(frames, views, ms[162], sb, over))
        over["scale"] = float(np.float32(255.5 / largest))
        check(gpu, scene, 162, 4, over, prm=fit.shape_params(min_points=1))
        over["scale"] = float(np.float32(4100.0 / radius))
        refused("mm from its origin", lambda: ft.shape_step_views(frames, views, ms[162], sb, over))
        # 2^23 terms: 1092 instances of three views of 2562 points in one subject; spread over two subjects they pass the count (and
        # are refused for the next reason, a set that does not exist, before anything runs)
        lots = np.repeat(inst[:1], 1092)
        refused("has more than 8388608 terms", lambda: ft.shape_step_views(frames, views, ms[2562], big, lots))
        st = np.zeros(1092, np.uint32)
        st[-1] = 2
        refused("names set 2 of 2", lambda: ft.shape_step_views(frames, views, ms[2562], big, lots, sets=st, subjects=np.arange(1092) % 2, n_subjects=2))
        one_view = lots.copy()
        one_view["views"] = 0b100
        refused("names set 2 of 2", lambda: ft.shape_step_views(frames, views, ms[2562], big, one_view, sets=st))       # 1092 pairs pass
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_lots = torch.from_numpy(one_view.view(np.uint8).copy()).cuda()
        refused("1092 instances of 3 views of 2562 points exceed", lambda: ft.shape_step_views(d_frames, views, ms[2562], big, d_lots, device_out=True))
        with pytest.raises(ValueError):
            ft.shape_step_views(frames[:, :2], views, ms[162], sb, inst)
