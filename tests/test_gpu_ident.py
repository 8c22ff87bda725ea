"""Identifying the subject of a fitted head on the GPU (k_ident.hip) against its restatement
tests/ident_ref.py: subjects, records, poses and every pair's score equal as bytes, with no tolerance.  Frames are splatted from a
subject's own model (tests/ident_scenes.py), 96x96 or 160x120, so a case costs little at any mesh size."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import fit_ref as fr
import ident_ref as ir
import ident_scenes as isc
import shape_scenes as ss
import surface_ref as su
import surface_scenes as us
from gpu_kit import to_device
from depthhead_amd import _lib, fit

pytestmark = pytest.mark.gpu

INST, REC, FREC, SREC = _lib.RENDER_INSTANCE_DTYPE, _lib.IDENT_RECORD_DTYPE, _lib.FIT_RECORD_DTYPE, _lib.SURFACE_RECORD_DTYPE
LDS = 1024                 # DH_FIT_LDS_POINTS: a model is staged up to it and streamed above
EINVAL = -1
SMALL = dict(min_points=16, max_rms=np.inf)


@pytest.fixture(scope="module")
def ft():
    with fit.Fitter() as f:
        yield f


@contextlib.contextmanager
def gpu_set(v, t, B, st):
    """The set on the GPU in the state of the restated one: its coefficients and, for a surface set, its offsets."""
    surface = hasattr(st, "offsets")
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, len(st), max_offset=16.0 if surface else None) as got:
        got.set_coeffs(st.state["coeffs"][:, :len(B)])
        if surface:
            for s in range(len(st)):
                got.set_offsets(s, st.offsets[s])
        for s in (0, len(st) - 1):
            pts, nrm = got.read(s)
            assert pts.tobytes() == st.pts[s].tobytes() and nrm.tobytes() == st.nrm[s].tobytes()
        yield got


def on_gpu(ft, got, frames, K, rec_in, n_subjects=None, enrolled=None, frec=None, prm=None, device=False):
    """(subjects u32, records, poses, scores [m, n_subjects]) from the host form, or from the _device form on the current stream."""
    if not device:
        return ft.identify_subjects(frames, got, rec_in, K, n_subjects=n_subjects, enrolled=enrolled, fit_records=frec, params=prm, scores=True)
    import torch
    d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
    d = ft.identify_subjects(d_frames, got, to_device(rec_in), K, n_subjects=n_subjects,
                             enrolled=None if enrolled is None else to_device(np.asarray(enrolled, np.uint8)),
                             fit_records=None if frec is None else to_device(frec), params=prm, scores=True, device_out=True)
    torch.cuda.synchronize()
    ns = len(got) if n_subjects is None else n_subjects
    return (d[0].cpu().numpy().view(np.uint32), d[1].cpu().numpy().view(REC), d[2].cpu().numpy().view(INST),
            d[3].cpu().numpy().view(FREC).reshape(len(rec_in), ns))


def same(got, want, what):
    subjects, rec, poses, scores = got
    w_subjects, w_rec, w_poses, w_scores = want
    assert subjects.tobytes() == w_subjects.tobytes(), (what, subjects, w_subjects)
    assert rec.tobytes() == w_rec.tobytes(), (what, rec, w_rec)
    assert scores.tobytes() == w_scores.tobytes(), (what, scores, w_scores)
    assert poses.tobytes() == ss.as_records(w_poses).tobytes(), (what, poses, w_poses)


def both(ft, got, st, frames, K, inst, prm_kw, what, n_subjects=None, enrolled=None, fit_status=None, device=False, Ks=None):
    """One identification on the GPU and in the restatement; everything equal.  Returns the restatement's answer."""
    frec = None
    if fit_status is not None:
        frec = np.zeros(len(inst), FREC)
        frec["status"] = fit_status
    out = on_gpu(ft, got, frames, K, ss.as_records(inst), n_subjects, enrolled, frec, fit.ident_params(**prm_kw), device)
    ref = ir.identify(frames, K if Ks is None else Ks, st, inst, n_subjects, enrolled, fit_status, ir.params(**prm_kw))
    same(out, ref, what)
    return ref


MESHES = [("4", 96, 96), ("255", 96, 96), ("256", 96, 96), ("257", 160, 120), ("strip%d" % (LDS - 1), 160, 120), ("strip%d" % LDS, 160, 120),
          ("strip%d" % (LDS + 1), 160, 120), ("2562", 160, 120)]


@pytest.mark.parametrize("name,w,h", MESHES)
def test_every_mesh_size_staged_and_streamed(ft, name, w, h):
    """4 vertices (below min_points: no candidate), the lane stride of a pass, the strip below, at and above the LDS budget, 2562
    vertices; three subjects, two heads; the host form and, for every other case, the _device form."""
    v, t, B, frames, K, inst, st = isc.gallery(name, 3, w, h, [0, 2])
    with gpu_set(v, t, B, st) as got:
        ref = both(ft, got, st, frames, K, inst, SMALL, name, device=name in ("255", "257", "strip%d" % LDS, "2562"))
        if name == "4":
            assert (ref[1]["status"] == ir.NO_CANDIDATE).all() and (ref[3]["status"] == fr.FEW_POINTS).all()
        else:
            assert (ref[1]["eligible"] >= 1).all() and (ref[1]["status"] == ir.OK).all(), ref[1]
            assert (ref[3]["steps"][ref[3]["status"] == fr.OK] > 0).all()


@pytest.mark.parametrize("n_subjects", [1, 2, 3, 63, 64, 65, 256])
def test_gallery_sizes_about_the_decide_waves_stride(ft, n_subjects):
    """S = 1 (no second), 2, 3, one below, at and above the 64 lanes of the decide wave, 256; every candidate eligible, so the
    best and the second come out of the whole reduction."""
    v, t, B, frames, K, inst, st = isc.gallery("642", n_subjects, 96, 96, [n_subjects // 2])
    with gpu_set(v, t, B, st) as got:
        ref = both(ft, got, st, frames, K, inst, SMALL, n_subjects, device=n_subjects in (2, 64, 256))
        assert ref[1]["eligible"][0] == n_subjects and ref[1]["status"][0] == ir.OK
        assert (ref[1]["second"][0] == ir.UNKNOWN) == (n_subjects == 1)


def test_fewer_subjects_than_the_set_and_the_enrolment_mask(ft):
    v, t, B, frames, K, inst, st = isc.gallery("642", 5, 96, 96, [0, 4, 2])
    with gpu_set(v, t, B, st) as got:
        ref = both(ft, got, st, frames, K, inst, SMALL, "n_subjects 3 of 5", n_subjects=3)
        assert ref[3].shape == (3, 3) and ref[0].tolist()[0] == 0 and 4 not in ref[0].tolist()
        for device in (False, True):
            ref = both(ft, got, st, frames, K, inst, SMALL, "a mask", enrolled=[1, 0, 0, 1, 1], device=device)
            assert not ref[3][:, 1:3].tobytes().strip(b"\0") and (ref[1]["eligible"] == 3).all() and ref[0].tolist() == [0, 4, 3]
            ref = both(ft, got, st, frames, K, inst, SMALL, "nobody enrolled", enrolled=[0] * 5, device=device)
            assert (ref[1]["status"] == ir.NO_CANDIDATE).all() and not ref[3].tobytes().strip(b"\0")


@pytest.mark.parametrize("n_inst", [0, 1, 33])
def test_instance_counts(ft, n_inst):
    v, t, B, frames, K, inst, st = isc.gallery("162", 2, 96, 96, [i % 2 for i in range(n_inst)], z=350.0)
    with gpu_set(v, t, B, st) as got:
        for device in (False, True):
            ref = both(ft, got, st, frames, K, inst, SMALL, n_inst, device=device)
            assert len(ref[0]) == n_inst and (ref[1]["status"] == ir.OK).all()


@pytest.mark.parametrize("iterations", [0, 1, 4, 64])
def test_iterations(ft, iterations):
    v, t, B, frames, K, inst, st = isc.gallery("642", 3, 96, 96, [0, 1, 2, 1])
    with gpu_set(v, t, B, st) as got:
        ref = both(ft, got, st, frames, K, inst, dict(SMALL, iterations=iterations), iterations, device=iterations in (0, 64))
        assert (ref[3]["steps"] <= iterations).all() and (ref[3]["steps"].max() == iterations or iterations == 64)
        if iterations == 0:
            assert ss.as_records(ref[2]).tobytes() == ss.as_records(inst).tobytes()
        if iterations == 4:
            assert ref[0].tolist() == [0, 1, 2, 1]


def test_a_pair_that_ends_few_points_and_one_that_ends_singular_among_eligible_ones(ft):
    v, t, B, frames, K, inst, st = isc.gallery("642", 3, 96, 96, [0, 1, 2, 1], z=350.0)
    with gpu_set(v, t, B, st) as got:
        ref = both(ft, got, st, frames, K, inst, dict(min_points=150, max_rms=np.inf), "few points", device=True)
        assert sorted(set(ref[3]["status"].reshape(-1).tolist())) == [fr.OK, fr.FEW_POINTS] and ref[0].tolist() == [0, 1, 2, 1]
        assert ref[1]["eligible"].tolist() == [2, 3, 2, 3]
    v, t, B, frames, K, inst, st = isc.flat_gallery()
    with gpu_set(v, t, B, st) as got:
        for device in (False, True):
            ref = both(ft, got, st, frames, K, inst, dict(SMALL, lam=0.0, iterations=3), "singular", device=device)
            assert ref[3]["status"][0].tolist() == [fr.SINGULAR, fr.OK] and ref[1][0]["best"] == 1 and ref[1][0]["eligible"] == 1


def test_two_identical_subjects_the_limit_from_both_sides_and_no_limit(ft):
    v, t, B, frames, K, inst, st = isc.gallery("642", 3, 96, 96, [1, 1])
    st.set_coeffs(np.array([[0.1], [0.1], [-0.4]]))
    with gpu_set(v, t, B, st) as got:
        for ratio, status in ((1.0, ir.OK), (1.5, ir.AMBIGUOUS)):
            ref = both(ft, got, st, frames, K, inst, dict(SMALL, min_ratio=ratio), ratio, device=ratio > 1)
            assert (ref[1]["status"] == status).all() and (ref[1]["best"] == 0).all() and (ref[1]["second"] == 1).all()
        m = float(ir.mean_square(ref[1]["sum_r2_best"][0], ref[1]["points_best"][0]))
        above, below = np.sqrt(m) * (1 + 1e-9), np.sqrt(m) * (1 - 1e-9)
        assert above * above >= m > below * below
        for max_rms, status in ((above, ir.OK), (below, ir.FAR), (np.inf, ir.OK), (1e-3, ir.FAR)):
            ref = both(ft, got, st, frames[:1], K, inst[:1], dict(min_points=16, max_rms=max_rms), max_rms)
            assert ref[1]["status"][0] == status and ref[1]["best"][0] == 0 and (ref[0][0] == 0) == (status == ir.OK)


def test_models_across_the_frame_edges_wholly_outside_and_instances_that_take_no_part(ft):
    """What the host forms refuse per instance, the device skips: a frame that does not exist, a NaN in t, an infinite R, an R
    outside the rotation tolerance (one inside it takes part), a scale that carries the set's bound past the extent limit; a fit
    record that is not OK is skipped by both forms."""
    v, t, B, frames, K, inst, st = isc.gallery("642", 3, 96, 96, [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2])
    f = float(K[0, 0])
    for i, (dx, dy) in enumerate([(-48, 0), (48, 0), (0, -48), (0, 48), (4000, 0), (0, -4000)]):   # pixels, at the pose's depth
        z = float(inst[i]["t"][2])
        inst[i]["t"] = inst[i]["t"] + np.array([dx * z / f, dy * z / f, 0.0], np.float32)
    with gpu_set(v, t, B, st) as got:
        for device in (False, True):
            ref = both(ft, got, st, frames, K, inst, SMALL, "edges", device=device)
            assert (ref[1]["status"][4:6] == ir.NO_CANDIDATE).all() and (ref[1]["status"][6:] == ir.OK).all()
        status = np.zeros(len(inst), np.uint32)
        status[[6, 9]] = (fr.FEW_POINTS, fr.SINGULAR)
        for device in (False, True):
            ref = both(ft, got, st, frames, K, inst, SMALL, "fit records", fit_status=status, device=device)
            assert ref[1]["status"][[6, 9]].tolist() == [ir.SKIPPED] * 2 and not ref[3][[6, 9]].tobytes().strip(b"\0")
        bad = [dict(i) for i in inst]
        bad[6]["frame"] = 99
        bad[7]["t"] = np.array([np.nan, 0.0, 800.0], np.float32)
        bad[8]["R"] = np.where(np.eye(3, dtype=bool), np.float32(np.inf), inst[8]["R"])
        bad[9]["R"] = (inst[9]["R"] * np.float32(1.02)).astype(np.float32)          # R R^T = 1.0404 I: outside the tolerance of 0.02
        bad[10]["R"] = (inst[10]["R"] * np.float32(1.005)).astype(np.float32)       # 1.010025 I: within it, takes part
        bad[11]["scale"] = np.float32(40.0)                                         # 40 * the bound (about 150 mm) > 4096
        ref = both(ft, got, st, frames, K, bad, SMALL, "faulty instances", device=True)
        assert ref[1]["status"][6:].tolist() == [ir.SKIPPED] * 4 + [ir.OK, ir.SKIPPED], ref[1]
        for i in (6, 7, 8, 9, 11):                                                  # skipped: the input copied through, bit for bit
            assert ref[0][i] == ir.UNKNOWN and ss.as_records(ref[2][i:i + 1]).tobytes() == ss.as_records(bad[i:i + 1]).tobytes()
        for host_bad, text in ((6, "names frame 99"), (7, "non-finite"), (8, "non-finite"), (9, "instance 9"), (11, "spans")):
            only = [dict(i) for i in inst]
            only[host_bad] = bad[host_bad]
            with pytest.raises(_lib.DepthheadError, match=text):
                ft.identify_subjects(frames, got, ss.as_records(only), K)
            skip = np.zeros(len(inst), FREC)                                        # ... unless its fit record says it takes no part
            skip["status"][host_bad] = fr.FEW_POINTS
            assert ft.identify_subjects(frames, got, ss.as_records(only), K, fit_records=skip)[1]["status"][host_bad] == ir.SKIPPED


def test_the_camera_twins_with_a_matrix_that_is_no_pinhole_on_a_surface_set(ft):
    from depthhead_amd import tracking
    v, t, B, frames, K, inst, st = isc.gallery("642", 3, 96, 96, [0, 1, 2, 1], surface=True)
    Ks = np.tile(np.asarray(K, np.float32), (len(frames), 1, 1))
    Ks[:, 0, 1] = 3.0                                      # a skew
    Ks[:, 2, 0] = 1e-5                                     # and a last row that is not (0, 0, 1)
    Ks[1::2, 0, 2] += 5.0
    with tracking.Cameras(Ks) as cams, gpu_set(v, t, B, st) as got:
        for device in (False, True):
            ref = both(ft, got, st, frames, cams, inst, SMALL, "cameras", device=device, Ks=Ks)
            assert (ref[1]["eligible"] == 3).all()
        plain = both(ft, got, st, frames, K, inst, SMALL, "one K")
        assert plain[3].tobytes() != ref[3].tobytes()


def test_host_form_against_the_device_form_after_a_device_fit_between_guard_bands_and_two_runs(ft):
    """The _device form on a side stream, fed by a device fit's instances and records, every output written between guard bands;
    the host form from the same fit read back; a second run of each: all equal the restatement."""
    import torch
    v, t, B, frames, K, inst, st = isc.gallery("642", 3, 96, 96, [0, 1, 2, 1, 0], nudge=(4.0, -3.0, 5.0))
    frames = frames.copy()
    frames[4] = 0                                                                   # the fit of instance 4 ends FEW_POINTS: skipped
    lib = _lib.load()
    with gpu_set(v, t, B, st) as got, fit.Model(st.pts[1], st.nrm[1]) as generic:
        m, ns = len(inst), 3
        stream = torch.cuda.Stream()
        band = 256
        sizes = {"sub": 4 * m, "rec": REC.itemsize * m, "poses": INST.itemsize * m, "scores": FREC.itemsize * m * ns}
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        Kf = np.ascontiguousarray(K, np.float32).reshape(9)
        runs = []
        for _ in range(2):
            out = {k: torch.full((2 * band + n,), 0xCD, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                d_inst, d_frec = ft.fit(d_frames, [generic], ss.as_records(inst), K, device_out=True, stream=stream.cuda_stream)
                fit.check(lib.dh_fit_identify_subjects_device(
                    ft._h, C.c_void_p(d_frames.data_ptr()), len(frames), 96, 96, _lib.vp(Kf), got._h, C.c_void_p(d_inst.data_ptr()), C.c_uint32(m), None,
                    C.c_uint32(ns), C.c_void_p(d_frec.data_ptr()), C.byref(fit.ident_params(**SMALL)), C.c_void_p(out["sub"].data_ptr() + band),
                    C.c_void_p(out["rec"].data_ptr() + band), C.c_void_p(out["poses"].data_ptr() + band), C.c_void_p(out["scores"].data_ptr() + band),
                    C.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            raw = {k: o.cpu().numpy() for k, o in out.items()}
            for k, r in raw.items():
                assert (r[:band] == 0xCD).all() and (r[-band:] == 0xCD).all(), k
            fitted, frec = d_inst.cpu().numpy().view(INST), d_frec.cpu().numpy().view(FREC)
            runs.append((fitted.tobytes(), frec.tobytes()) + tuple(raw[k][band:-band].tobytes() for k in sizes))
        assert runs[0] == runs[1]
        assert frec["status"].tolist() == [fr.OK] * 4 + [fr.FEW_POINTS]
        ref_inst = [us.instance(int(r["frame"]), r["R"].reshape(3, 3), r["t"], r["scale"]) for r in fitted]
        ref = ir.identify(frames, K, st, ref_inst, None, None, frec["status"], ir.params(**SMALL))
        dev = (raw["sub"][band:-band].view(np.uint32), raw["rec"][band:-band].view(REC), raw["poses"][band:-band].view(INST),
               raw["scores"][band:-band].view(FREC).reshape(m, ns))
        same(dev, ref, "device form")
        assert ref[1]["status"].tolist() == [ir.OK] * 4 + [ir.SKIPPED] and ref[0].tolist() == [0, 1, 2, 1, ir.UNKNOWN]
        for _ in range(2):
            same(ft.identify_subjects(frames, got, fitted, K, fit_records=frec, params=fit.ident_params(**SMALL), scores=True), ref, "host form")


def test_no_poses_and_no_scores(ft):
    """poses_out NULL and scores NULL, in both forms: the subjects and the records are what they are with them."""
    import torch
    v, t, B, frames, K, inst, st = isc.gallery("642", 3, 96, 96, [2, 0])
    lib, vp = _lib.load(), _lib.vp
    ref = ir.identify(frames, K, st, inst, prm=ir.params(**SMALL))
    rin, Kf, prm = ss.as_records(inst), np.ascontiguousarray(K, np.float32).reshape(9), fit.ident_params(**SMALL)
    with gpu_set(v, t, B, st) as got:
        sub, rec = np.zeros(2, np.uint32), np.zeros(2, REC)
        fit.check(lib.dh_fit_identify_subjects(ft._h, vp(frames), 2, 96, 96, vp(Kf), got._h, vp(rin), C.c_uint32(2), None, C.c_uint32(3), None, C.byref(prm),
                                               vp(sub), vp(rec), None, None))
        assert sub.tobytes() == ref[0].tobytes() and rec.tobytes() == ref[1].tobytes()
        d_frames, d_in = torch.from_numpy(frames.view(np.int16).copy()).cuda(), to_device(rin)
        d_sub, d_rec = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2 * REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fit.check(lib.dh_fit_identify_subjects_device(ft._h, C.c_void_p(d_frames.data_ptr()), 2, 96, 96, vp(Kf), got._h, C.c_void_p(d_in.data_ptr()),
                                                      C.c_uint32(2), None, C.c_uint32(3), None, C.byref(prm), C.c_void_p(d_sub.data_ptr()),
                                                      C.c_void_p(d_rec.data_ptr()), None, None, None))
        torch.cuda.synchronize()
        assert d_sub.cpu().numpy().tobytes() == ref[0].tobytes() and d_rec.cpu().numpy().tobytes() == ref[1].tobytes()


def test_the_answer_of_the_device_form_chained_into_a_device_surface_step(ft):
    """subjects_out and poses_out of the _device form handed, on the same stream and unread, to dh_fit_surface_subjects_device as
    its subjects and instances: the unknown head takes no part, and the set ends where the restated chain ends."""
    import torch
    truth = [0, 1, 2, 1, 0, 2]
    v, t, B, frames, K, inst, st = isc.gallery("642", 3, 96, 96, truth, surface=True)
    frames = frames.copy()
    frames[3] = 0                                                                   # an unknown head
    with gpu_set(v, t, B, st) as got:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_sub, d_rec, d_poses = ft.identify_subjects(d_frames, got, to_device(ss.as_records(inst)), K, params=fit.ident_params(**SMALL), device_out=True)
        d_srec = ft.surface_step_subjects(d_frames, got, d_poses, K, subjects=d_sub, params=fit.surface_params(min_points=1), device_out=True)
        torch.cuda.synchronize()
        subjects, rec, poses, _ = ir.identify(frames, K, st, inst, prm=ir.params(**SMALL))
        assert subjects.tolist() == [0, 1, 2, ir.UNKNOWN, 0, 2]
        assert d_sub.cpu().numpy().view(np.uint32).tobytes() == subjects.tobytes() and d_rec.cpu().numpy().tobytes() == rec.tobytes()
        srec = su.surface_step(frames, K, st, poses, subjects, 3, None, su.params(min_points=1))
        assert d_srec.cpu().numpy().tobytes() == srec.tobytes() and srec["instances"].tolist() == [2, 1, 2]
        for s in range(3):
            pts, nrm = got.read(s)
            assert got.offsets(s).tobytes() == st.offsets[s].tobytes() and pts.tobytes() == st.pts[s].tobytes() and nrm.tobytes() == st.nrm[s].tobytes()


def test_recognise_subjects_against_the_restated_driver_on_the_evaluations_probes(ft):
    """fit.recognise_subjects over the 16 probes of the evaluation -- 12 of enrolled subjects, 4 of a stranger -- with the shipped
    defaults: the bytes of tests/ident_ref.py, and with them 12 right answers and 4 times DH_IDENT_FAR."""
    st, enrolled, K, probes, starts, truth = isc.evaluation()
    want_sub, want_rec, want_poses, want_frec = isc.evaluation_result()
    v, t, n, B = us.eval_generic()
    with gpu_set(v, t, B, st) as got, fit.Model(v, n) as generic:
        subjects, rec, poses, frec = fit.recognise_subjects(ft, probes, K, got, ss.as_records(starts), generic, enrolled=enrolled)
        assert subjects.tobytes() == want_sub.tobytes() and rec.tobytes() == want_rec.tobytes(), (subjects, rec, want_rec)
        assert poses.tobytes() == ss.as_records(want_poses).tobytes()
        assert [int(r["status"]) for r in want_frec] == frec["status"].tolist() and [int(r["sum_r2_fixed"]) for r in want_frec] == frec["sum_r2_fixed"].tolist()
        assert subjects.tolist() == [ir.UNKNOWN if who is None else who for who in truth]
        assert rec["status"].tolist() == [ir.FAR if who is None else ir.OK for who in truth]
        empty = fit.recognise_subjects(ft, probes, K, got, ss.as_records([]), generic, enrolled=enrolled)
        assert [len(x) for x in empty] == [0, 0, 0, 0]
