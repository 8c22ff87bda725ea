"""The shape step on the GPU (k_fit_shape.hip) against its restatement tests/shape_ref.py: every field of
every dh_shape_record equal, with no tolerance.  Scenes are those of tests/shape_scenes.py and tests/fit_scenes.py; what is
compared is the arithmetic, so the instances are true or rough poses wherever a fitted one is not what the test is about."""
import ctypes as C
import functools

import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import render_ref as rr
import shape_ref as sr
import shape_scenes as ss
from gpu_kit import fit_models, same_records
from depthhead_amd import _lib, fit, render, synth

pytestmark = pytest.mark.gpu

INST, REC = _lib.RENDER_INSTANCE_DTYPE, _lib.SHAPE_RECORD_DTYPE
W, H = 160, 120
SIZES = (162, 1, 255, 256, 257, 2562)


def fields8(v, n):
    """Eight fields of a model: head_basis's four, three shears and 10 mm along the normal."""
    v = np.asarray(v, np.float64)
    z = np.zeros(len(v))
    extra = [np.stack([v[:, 1], z, z], 1), np.stack([z, v[:, 2], z], 1), np.stack([z, z, v[:, 0]], 1), 10.0 * np.asarray(n, np.float64)]
    return np.concatenate([synth.head_basis(v), np.array(extra, np.float32)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_models():
    """points -> (pts, nrm, fields [8, points, 3]): head_mesh(2) whole (162), head_mesh(4) whole (2562) and its first 255, 256 and
    257 points -- either side of the workgroup's 256 lanes, a wave's tail -- and one point that faces the camera."""
    v2, _, n2 = fs.head(2)
    v4, _, n4 = fs.head(4)
    B2, B4 = fields8(v2, n2), fields8(v4, n4)
    front = int(np.argmin(v2[:, 2]))
    out = {162: (v2, n2, B2), 2562: (v4, n4, B4), 1: (v2[front:front + 1].copy(), n2[front:front + 1].copy(), B2[:, front:front + 1].copy())}
    for k in (255, 256, 257):
        out[k] = (v4[:k].copy(), n4[:k].copy(), B4[:, :k].copy())
    return out


@pytest.fixture(scope="module")
def gpu():
    with fit_models(host_models()) as both:
        yield both


def ref_params(prm):
    return sr.params() if prm is None else sr.params(prm.gate, prm.lam, prm.min_points)


def same(got, want, what):
    assert got.dtype == REC
    same_records(got, want, what)


def check(gpu, frames, K, points, nk, inst, subjects=None, ns=1, prm=None, K_gpu=None):
    """One host call on model `points` with its first nk fields, against the restatement."""
    ms, ft = gpu
    pts, nrm, B = host_models()[points]
    with fit.ShapeBasis(B[:nk]) as sb:
        got = ft.shape_step(frames, ms[points], sb, inst, K if K_gpu is None else K_gpu, subjects=subjects, n_subjects=ns, params=prm)
    want = sr.shape_step(frames, K, pts, nrm, B[:nk], inst, subjects, ns, ref_params(prm))
    same(got, want, "record")
    return got


@functools.lru_cache(maxsize=None)
def subject_instances(seed=0):
    """(frames [8, H, W], K, instances [16]): the subject's true poses, then its rough starts."""
    frames, K, pos, Rs = ss.subject(W, H, seed)
    inst = ss.as_records(ss.true_instances(pos, Rs) + ss.rough_instances(seed, pos, Rs))
    inst["flags"] = 0x5A0000 + np.arange(len(inst))      # ignored by the step
    inst["mesh"][1::2] = 7                               # ignored too: a call has one model
    inst.setflags(write=False)
    return frames, K, inst


def test_one_instance_96x96_one_field(gpu):
    frame, K, pos, R = fs.scene(96, 96, 7100)
    inst = ss.as_records([{"frame": 0, "R": R, "t": pos, "scale": 1.0}])
    rec = check(gpu, frame[None], K, 162, 1, inst, prm=fit.shape_params(min_points=16))
    assert rec["status"][0] == fit.SHAPE_OK and rec["points"][0] >= 30 and rec["instances"][0] == 1
    assert abs(rec["delta"][0, 0]) < 0.1 and (rec["delta"][0, 1:] == 0.0).all() and rec["sum_r2_fixed"][0] > 0


@pytest.mark.parametrize("nk", range(1, 9))
def test_field_counts(gpu, nk):
    frames, K, inst = subject_instances()
    rec = check(gpu, frames, K, 162, nk, inst[:8])
    assert rec["status"][0] == fit.SHAPE_OK and rec["instances"][0] == 8 and (rec["delta"][0, :nk] != 0.0).all() and (rec["delta"][0, nk:] == 0.0).all()
    if nk >= 3:
        assert (np.sign(rec["delta"][0, :3]) == np.sign(ss.C_TRUE[:3])).all()


@pytest.mark.parametrize("points", SIZES[1:])
def test_model_sizes(gpu, points):
    frames, K, inst = subject_instances()
    rec = check(gpu, frames, K, points, 4, inst, prm=fit.shape_params(min_points=1))
    assert rec["points"][0] > 0 and rec["status"][0] in (fit.SHAPE_OK, fit.SHAPE_SINGULAR)
    if points == 2562:
        assert rec["status"][0] == fit.SHAPE_OK and rec["points"][0] > 16 * 500 and rec["instances"][0] == 16


def test_twelve_instances_over_five_frames_in_three_subjects(gpu):
    """Subject 1 has no instance, instances 3 and 8 are skipped, frame 4 is empty (its instance associates nothing)."""
    sub, K, inst = subject_instances()
    frames = np.concatenate([sub[:4], np.zeros((1, H, W), np.uint16)])
    pick = [0, 1, 2, 3, 8, 9, 10, 11, 0, 1, 2, 3]
    twelve = inst[pick].copy()
    twelve["t"][8:, 0] += np.float32(3.0)
    twelve["frame"][11] = 4
    subjects = np.array([0, 0, 2, sr.SKIP, 2, 2, 0, 0, sr.SKIP, 2, 0, 2], np.uint32)
    rec = check(gpu, frames, K, 162, 4, twelve, subjects, 3)
    assert rec["status"].tolist() == [fit.SHAPE_OK, fit.SHAPE_FEW_POINTS, fit.SHAPE_OK]
    assert rec["instances"].tolist() == [5, 0, 4] and rec["points"][1] == 0 and (rec["delta"][1] == 0.0).all()
    # skipped instances change nothing, and neither does what a skipped instance holds
    keep = subjects != sr.SKIP
    same(check(gpu, frames, K, 162, 4, twelve[keep], subjects[keep], 3), rec, "without the skipped")
    junk = twelve.copy()
    junk["t"][3] = (1e30, np.nan, 0.0); junk["frame"][8] = 4000; junk["R"][8] = np.inf
    ms, ft = gpu
    with fit.ShapeBasis(host_models()[162][2][:4]) as sb:
        same(ft.shape_step(frames, ms[162], sb, junk, K, subjects=subjects, n_subjects=3), rec, "junk in the skipped")
        # two subjects in one call are two calls
        for sj in (0, 2):
            one = ft.shape_step(frames, ms[162], sb, twelve[subjects == sj], K)
            assert one[0].tobytes() == rec[sj].tobytes()


@functools.lru_cache(maxsize=None)
def many(count):
    """`count` instances of the subject's eight frames, each true pose moved by a few seeded millimetres."""
    frames, K, inst = subject_instances()
    out = inst[np.arange(count) % 8].copy()
    out["t"] += (6.0 * synth.SplitMix(4242).uniform(3 * count).reshape(count, 3) - 3.0).astype(np.float32)
    out.setflags(write=False)
    return frames, K, out


@pytest.mark.parametrize("count", (1, 255, 257))
def test_instance_counts_into_one_subject(gpu, count):
    frames, K, inst = many(count)
    rec = check(gpu, frames, K, 162, 4, inst, prm=fit.shape_params(min_points=16))
    assert rec["status"][0] == fit.SHAPE_OK and rec["instances"][0] == count and rec["points"][0] > 30 * count


def test_camera_table_with_a_matrix_that_is_no_pinhole(gpu):
    from depthhead_amd.tracking import Cameras
    ms, ft = gpu
    n = 3
    K = synth.default_intrinsic(W, H)
    Ks = np.stack([K, K, K]).astype(np.float32)
    Ks[1, 0, 0] *= 1.3; Ks[1, 1, 1] *= 0.8; Ks[1, 0, 2] += 11.5
    Ks[2, 0, 1] = 3.0; Ks[2, 2, 0] = 1e-4                             # a matrix that is no pinhole
    v, t, _ = ss.subject_mesh()
    poses = [(render.euler_to_matrix((3, 20, -8)), (30.0, -10.0, 850.0)), (render.euler_to_matrix((-5, -30, 10)), (-60.0, 15.0, 1000.0)),
             (render.euler_to_matrix((8, 10, 15)), (10.0, 20.0, 900.0))]
    frames, _ = rr.render([(v, t)], [rr.instance(f, 0, R, p) for f, (R, p) in enumerate(poses)], n, W, H, Ks, noise=2, holes=0.02, seed=8)
    inst = ss.as_records([{"frame": f, "R": R, "t": np.float32(p), "scale": 1.0} for f, (R, p) in enumerate(poses)])
    with Cameras(Ks) as cams:
        rec = check(gpu, frames, Ks, 162, 4, inst, K_gpu=cams)
        with fit.ShapeBasis(host_models()[162][2][:4]) as sb:
            with pytest.raises(_lib.DepthheadError) as ei:
                ft.shape_step(frames[:2], ms[162], sb, inst[:2], cams)
            assert ei.value.code == -1 and "holds 3 cameras" in str(ei.value)
            one = ft.shape_step(frames, ms[162], sb, inst, K)
    assert rec["status"][0] == fit.SHAPE_OK and rec["instances"][0] == 3
    assert one[0].tobytes() != rec[0].tobytes()


def test_gates_and_min_points(gpu):
    frames, K, inst = subject_instances()
    narrow = check(gpu, frames, K, 162, 4, inst, prm=fit.shape_params(gate=1.0, min_points=1))
    wide = check(gpu, frames, K, 162, 4, inst, prm=fit.shape_params(gate=256.0))
    usual = check(gpu, frames, K, 162, 4, inst)
    assert 0 < narrow["points"][0] < usual["points"][0] < wide["points"][0]
    count = int(usual["points"][0])
    at = check(gpu, frames, K, 162, 4, inst, prm=fit.shape_params(min_points=count))
    above = check(gpu, frames, K, 162, 4, inst, prm=fit.shape_params(min_points=count + 1))
    assert at.tobytes() == usual.tobytes()
    assert above["status"][0] == fit.SHAPE_FEW_POINTS and (above["delta"] == 0.0).all()
    assert (above["points"][0], above["instances"][0], above["sum_r2_fixed"][0]) == (count, 16, usual["sum_r2_fixed"][0])


def test_both_exits(gpu):
    """FEW_POINTS: an empty frame.  SINGULAR: two identical fields with lambda = 0 over 257 instances, where the diagonal has
    grown past 2^53 * 1e-9 so that a + 1e-9 == a and the second pivot is a - (a / a) * a = 0; over 8 instances the same basis
    goes on by the 1e-9 term (tests/test_shape_ref.py)."""
    ms, ft = gpu
    frames, K, inst = many(257)
    pts, nrm, B = host_models()[162]
    twin = np.stack([B[0], B[0]])
    prm = fit.shape_params(lam=0.0)
    with fit.ShapeBasis(twin) as sb:
        empty = ft.shape_step(np.zeros_like(frames), ms[162], sb, inst, K, params=prm)
        same(empty, sr.shape_step(np.zeros_like(frames), K, pts, nrm, twin, inst, prm=ref_params(prm)), "empty")
        assert (empty["status"][0], empty["points"][0], empty["instances"][0], empty["sum_r2_fixed"][0]) == (fit.SHAPE_FEW_POINTS, 0, 0, 0)
        got = ft.shape_step(frames, ms[162], sb, inst, K, params=prm)
        same(got, sr.shape_step(frames, K, pts, nrm, twin, inst, prm=ref_params(prm)), "twin fields, 257 instances")
        assert got["status"][0] == fit.SHAPE_SINGULAR and (got["delta"] == 0.0).all() and got["points"][0] > 0
        few = ft.shape_step(frames, ms[162], sb, inst[:8], K, params=prm)
        same(few, sr.shape_step(frames, K, pts, nrm, twin, inst[:8], prm=ref_params(prm)), "twin fields, 8 instances")
        assert few["status"][0] == fit.SHAPE_OK


GUARD = 4096


def test_device_twins_chained_after_a_device_fit(gpu):
    """dh_fit_depth_device, then dh_fit_shape_device and its camera twin on the fitted instances, on a side stream with no host
    copy or wait between them; the records lie between 4 KB guard bands at a pointer that is 8 bytes off a 256-byte line.  A
    device instance the host forms would refuse (frame 999) is skipped on the device."""
    import torch
    from depthhead_amd.tracking import Cameras
    ms, ft = gpu
    frames, K, inst = subject_instances()
    pts, nrm, B = host_models()[162]
    starts = inst[8:].copy()
    starts["mesh"] = 0
    subjects = np.array([0, 1, 0, 1, 0, 1, 0, sr.SKIP], np.uint32)
    ns, bytes_ = 2, 2 * REC.itemsize
    stream = torch.cuda.Stream()
    with fit.ShapeBasis(B[:4]) as sb, Cameras(np.tile(K.reshape(1, 9), (8, 1))) as cams:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_subj = torch.from_numpy(subjects.view(np.int32).copy()).cuda()
        bufs = [torch.full((GUARD + 8 + bytes_ + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            d_out, d_rec = ft.fit(d_frames, [ms[162]], starts, K, device_out=True, stream=stream.cuda_stream)
            for buf, kind, karg in ((bufs[0], "", _lib.vp(np.ascontiguousarray(K, np.float32).reshape(9))), (bufs[1], "_cameras", cams._h)):
                rc = getattr(ft._lib, "dh_fit_shape" + kind + "_device")(
                    ft._h, C.c_void_p(d_frames.data_ptr()), 8, W, H, karg, ms[162]._h, sb._h, C.c_void_p(d_out.data_ptr()), C.c_uint32(8),
                    C.c_void_p(d_subj.data_ptr()), C.c_uint32(ns), None, C.c_void_p(buf.data_ptr() + GUARD + 8), C.c_void_p(stream.cuda_stream))
                _lib.check(rc)
        stream.synchronize()
        fitted = d_out.cpu().numpy().view(INST)
        status = d_rec.cpu().numpy().view(_lib.FIT_RECORD_DTYPE)["status"]
        host = ft.shape_step(frames, ms[162], sb, fitted, K, subjects=subjects, n_subjects=ns)
        want = sr.shape_step(frames, K, pts, nrm, B[:4], fitted, subjects, ns)
        same(host, want, "host form on the fitted instances")
        for buf in bufs:
            raw = buf.cpu().numpy()
            assert (raw[:GUARD + 8] == 0xEE).all() and (raw[GUARD + 8 + bytes_:] == 0xEE).all()
            same(raw[GUARD + 8:GUARD + 8 + bytes_].copy().view(REC), want, "device form")
        # an instance that names no frame: refused by the host form, skipped by the device
        bad = fitted.copy()
        bad["frame"][2] = 999
        with pytest.raises(_lib.DepthheadError) as ei:
            ft.shape_step(frames, ms[162], sb, bad, K, subjects=subjects, n_subjects=ns)
        assert ei.value.code == -1 and "names frame 999 of 8" in str(ei.value)
        d_bad = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
        got = ft.shape_step(d_frames, ms[162], sb, d_bad, K, subjects=d_subj, n_subjects=ns, device_out=True)
        torch.cuda.synchronize()
        skipped = subjects.copy()
        skipped[2] = sr.SKIP
        same(got.cpu().numpy().view(REC), sr.shape_step(frames, K, pts, nrm, B[:4], fitted, skipped, ns), "frame 999 skipped")
    assert (status == fit.FIT_OK).all() and want["status"].tolist() == [fit.SHAPE_OK, fit.SHAPE_OK] and want["instances"].tolist() == [4, 3]


def test_a_fitter_reused_with_a_smaller_a_larger_and_an_empty_call_and_fit_unchanged(gpu):
    """Also: Fitter.fit gives the same bytes before and after shape calls on the same fitter, and one call run twice the same
    bytes."""
    ms, _ = gpu
    frames, K, inst = subject_instances()
    pts, nrm, B = host_models()[162]
    small_f, small_K, pos, R = fs.scene(96, 96, 7100)
    small = ss.as_records([{"frame": 0, "R": R, "t": pos, "scale": 1.0}])
    prm = fit.shape_params(min_points=16)
    want_small = sr.shape_step(small_f[None], small_K, pts, nrm, B[:4], small, prm=ref_params(prm))
    want_large = sr.shape_step(frames, K, pts, nrm, B[:4], inst, np.arange(16, dtype=np.uint32) % 3, 3)
    starts = inst[8:].copy()
    starts["mesh"] = 0
    with fit.Fitter() as ft, fit.ShapeBasis(B[:4]) as sb:
        before = ft.fit(frames, [ms[162]], starts, K)
        for _ in range(2):
            same(ft.shape_step(small_f[None], ms[162], sb, small, small_K, params=prm), want_small, "small")
            same(ft.shape_step(frames, ms[162], sb, inst, K, subjects=np.arange(16) % 3, n_subjects=3), want_large, "large")
        none = ft.shape_step(frames, ms[162], sb, inst[:0], K, n_subjects=2)
        assert none["status"].tolist() == [fit.SHAPE_FEW_POINTS] * 2 and not none["points"].any() and not none["delta"].any()
        same(none, sr.shape_step(frames, K, pts, nrm, B[:4], inst[:0], n_subjects=2), "empty call")
        after = ft.fit(frames, [ms[162]], starts, K)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()


def test_one_call_captured_in_a_graph_and_replayed_twice(gpu):
    """The eager call first (it takes the fitter's sums buffer), then the capture, then two replays, each equal to the
    restatement.  With the sums cleared by hipMemsetAsync this case failed on an MI355X: the eager call equal, the first replay
    not (subject 0: 6763 points for 413); the cause was not found, the clear is a kernel since, and that build has not run on a
    GPU yet."""
    import torch
    ms, ft = gpu
    frames, K, inst = subject_instances()
    pts, nrm, B = host_models()[162]
    want = sr.shape_step(frames, K, pts, nrm, B[:4], inst, np.arange(16, dtype=np.uint32) % 2, 2)
    with fit.ShapeBasis(B[:4]) as sb:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_inst = torch.from_numpy(inst.view(np.uint8).copy()).cuda()
        d_subj = torch.from_numpy((np.arange(16) % 2).astype(np.int32)).cuda()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            eager = ft.shape_step(d_frames, ms[162], sb, d_inst, K, subjects=d_subj, n_subjects=2, device_out=True)   # takes the sums buffer
        stream.synchronize()
        same(eager.cpu().numpy().view(REC), want, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            rec = ft.shape_step(d_frames, ms[162], sb, d_inst, K, subjects=d_subj, n_subjects=2, device_out=True)
        for _ in range(2):
            rec.fill_(0xEE)
            g.replay()
            torch.cuda.synchronize()
            same(rec.cpu().numpy().view(REC), want, "replay")


def test_refusals_that_need_a_model(gpu):
    ms, ft = gpu
    frames, K, inst = subject_instances()
    pts, nrm, B = host_models()[162]

    def refused(what, fn):
        with pytest.raises(_lib.DepthheadError) as ei:
            fn()
        assert ei.value.code == -1 and what in str(ei.value), str(ei.value)

    with fit.ShapeBasis(B[:4]) as sb, fit.ShapeBasis(host_models()[2562][2][:2]) as big:
        n, k, largest = sb.info()
        assert (n, k) == (162, 4) and abs(largest - np.sqrt((B[:4].astype(np.float64) ** 2).sum(axis=2).max())) < 1e-9
        refused("the basis is one of 2562 points, the model has 162", lambda: ft.shape_step(frames, ms[162], big, inst, K))
        over = inst[:1].copy()
        for scale in (float(np.float32(256.5 / largest)), -float(np.float32(256.5 / largest))):
            over["scale"] = scale
            refused("scales the basis to", lambda: ft.shape_step(frames, ms[162], sb, over, K))
        over["scale"] = float(np.float32(255.5 / largest))
        check(gpu, frames, K, 162, 4, over, prm=fit.shape_params(min_points=1))
        # 2^23 terms: 3275 instances of 2562 points in one subject; spread over two subjects they pass the count (and are refused
        # for the next reason, a frame that does not exist, before anything runs)
        lots = np.repeat(inst[:1], 3275)
        refused("has more than 8388608 terms", lambda: ft.shape_step(frames, ms[2562], big, lots, K))
        lots["frame"][-1] = 8
        refused("names frame 8 of 8", lambda: ft.shape_step(frames, ms[2562], big, lots, K, subjects=np.arange(3275) % 2, n_subjects=2))
        import torch
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_lots = torch.from_numpy(lots.view(np.uint8).copy()).cuda()
        refused("3275 instances of 2562 points exceed", lambda: ft.shape_step(d_frames, ms[2562], big, d_lots, K, device_out=True))


def test_adapt_is_the_restated_adapt(gpu):
    """fit.adapt, two rounds, against shape_ref.adapt: the coefficients and the fitted instances to the bit."""
    _, ft = gpu
    v, t, _, B = ss.generic()
    frames, K, pos, Rs = ss.subject(W, H, 12)
    starts = ss.rough_instances(12, pos, Rs)
    c, inst, trace = fit.adapt(ft, frames, K, v, t, B, ss.as_records(starts), rounds=2)
    want_c, want_inst, want_trace = sr.adapt(frames, K, v, t, B, starts, fit.vertex_normals, rounds=2)
    assert c.tobytes() == want_c.tobytes() and len(trace) == 2
    assert inst.tobytes() == ss.as_records(want_inst).tobytes()
    for got, (wc, _, wrec) in zip(trace, want_trace):
        assert got["coeffs"].tobytes() == wc.tobytes() and got["shape"].tobytes() == wrec.tobytes()
    assert (np.sign(c[:3]) == np.sign(ss.C_TRUE[:3])).all()
