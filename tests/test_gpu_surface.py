"""A surface per subject on the GPU (k_surface.hip) against its restatement tests/surface_ref.py: every
offset, count, record, point, normal and state equal, with no tolerance.  Frames are splatted from a displaced copy of the mesh
(tests/surface_scenes.py), 96x96 or 160x120, so a case costs little at any mesh size."""
import ctypes as C
import functools

import numpy as np
import pytest

import fit_ref as fr
import shape_scenes as ss
import subjects_ref as sb
import subjects_scenes as sc
import surface_ref as su
import surface_scenes as us
from gpu_kit import to_device
from depthhead_amd import _lib, fit, synth

pytestmark = pytest.mark.gpu

INST, REC, FREC = _lib.RENDER_INSTANCE_DTYPE, _lib.SURFACE_RECORD_DTYPE, _lib.FIT_RECORD_DTYPE
LDS = _lib.SURFACE_LDS_POINTS
EINVAL = -1


@functools.lru_cache(maxsize=None)
def mesh(name):
    """name -> (verts, tris, one seeded field): 4, 255, 256, 257, 2562 and 10242 vertices, the fan, and strips of any size."""
    if name.startswith("strip"):
        v, t = us.strip_mesh(int(name[5:]))
    else:
        tetra = (np.array([(0, 0, 0), (40, 0, 0), (0, 40, 0), (0, 0, 40)], np.float32), np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.uint32))
        v, t = {"4": lambda: tetra, "255": lambda: sc.lathe_mesh(11, 23), "256": lambda: sc.lathe_mesh(2, 127), "257": lambda: sc.lathe_mesh(15, 17),
                "2562": lambda: synth.head_mesh(4), "10242": lambda: synth.head_mesh(5), "fan": sc.fan_mesh, "162": lambda: synth.head_mesh(2)}[name]()
    return v, t, 0.1 * sc.seeded_fields(v, 1, 40 + len(v))


def records(instances):
    return ss.as_records(instances)


def displacement(v, seed, height=6.0):
    """A seeded smooth displacement [n] (mm): two bumps of opposite sign."""
    u = synth.SplitMix(seed).uniform(2)
    extent = float(np.ptp(v, axis=0).max())
    return us.bump(v, int(u[0] * len(v)), height, 0.15 * extent) - us.bump(v, int(u[1] * len(v)), 0.7 * height, 0.1 * extent)


def same(got, want, what):
    """The set on the GPU (a fit.Subjects) against the restated one: every state, point, normal, offset and count."""
    state = got.state()
    assert state.tobytes() == want.state.tobytes(), (what, state, want.state)
    for s in range(len(want)):
        pts, nrm = got.read(s)
        o, c = got.offsets(s, counts=True)
        assert o.tobytes() == want.offsets[s].tobytes(), (what, "offsets", s, int((o != want.offsets[s]).sum()))
        assert (c == want.counts[s]).all(), (what, "counts", s)
        assert pts.tobytes() == want.pts[s].tobytes(), (what, "points", s, int((pts != want.pts[s]).sum()))
        assert nrm.tobytes() == want.nrm[s].tobytes(), (what, "normals", s, int((nrm != want.nrm[s]).sum()))


def scene(name, n_subjects, w, h, per_subject=2, seed=3, max_offset=16.0, coeffs=True):
    """(v, t, B, frames, K, instances, subject_of, the restated set): `per_subject` frames of every subject, each splatted from the
    base mesh displaced by the subject's own seeded bumps."""
    v, t, B = mesh(name)
    want = su.Set(v, t, B, n_subjects, max_offset=max_offset)
    frames, inst, who = [], [], []
    for s in range(n_subjects):
        f, K, ins = us.splat_scene(v, want.nb, displacement(v, seed + s), w, h, per_subject, seed + s)
        for it in ins:
            inst.append(dict(it, frame=it["frame"] + len(frames) * per_subject))
            who.append(s)
        frames.append(f)
    return v, t, B, np.concatenate(frames), K, inst, np.array(who, np.uint32), want


def step_both(ft, got, want, frames, K, inst, who, prm_kw, what, n_subjects=None, fit_status=None, device=False):
    """One surface step on the GPU (host form, or the _device form on the current stream) and in the restatement; everything equal."""
    import torch
    prm, ref_prm = fit.surface_params(**prm_kw), su.params(**prm_kw)
    rec_in = records(inst)
    frec = None
    if fit_status is not None:
        frec = np.zeros(len(inst), FREC)
        frec["status"] = fit_status
    if device:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_rec = ft.surface_step_subjects(d_frames, got, to_device(rec_in), K, subjects=torch.from_numpy(who.view(np.int32).copy()).cuda(),
                                         n_subjects=n_subjects, fit_records=None if frec is None else to_device(frec), params=prm, device_out=True)
        torch.cuda.synchronize()
        rec = d_rec.cpu().numpy().view(REC)
    else:
        rec = ft.surface_step_subjects(frames, got, rec_in, K, subjects=who, n_subjects=n_subjects, fit_records=frec, params=prm)
    ref = su.surface_step(frames, K, want, inst, who, n_subjects, None if frec is None else frec["status"], ref_prm)
    assert rec.tobytes() == ref.tobytes(), (what, rec, ref)
    same(got, want, what)
    return ref


@pytest.fixture(scope="module")
def ft():
    with fit.Fitter() as f:
        yield f


SMALL = dict(min_points=1)
CASES = [("4", 3, 96, 96), ("255", 3, 160, 120), ("256", 1, 96, 96), ("257", 65, 96, 96), ("2562", 3, 160, 120), ("fan", 3, 96, 96),
         ("strip%d" % (LDS - 1), 1, 160, 120), ("strip%d" % LDS, 3, 160, 120), ("strip%d" % (LDS + 1), 1, 160, 120), ("10242", 3, 160, 120)]


@pytest.mark.parametrize("name,n_subjects,w,h", CASES)
def test_a_step_over_every_mesh_size_and_both_solve_paths(ft, name, n_subjects, w, h):
    """4 .. 10242 vertices, the fan, the strip at the solve's LDS threshold, one below and one above; S = 1, 3 and 65; both frame
    sizes; the host form and, for three of the cases, the _device form; the models at non-zero coefficients."""
    v, t, B, frames, K, inst, who, want = scene(name, n_subjects, w, h)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, n_subjects, max_offset=16.0) as got:
        assert got.info() == (len(v), len(t), 1, n_subjects, float(want.radius), 0)
        same(got, want, "created")
        c = np.linspace(-0.3, 0.3, n_subjects).reshape(-1, 1)
        got.set_coeffs(c)
        want.set_coeffs(c)
        ref = step_both(ft, got, want, frames, K, inst, who, SMALL, name, device=name in ("255", "2562", "strip%d" % LDS))
        assert (ref["status"] == su.OK).all() and ref["observed"].sum() > 0 and ref["max_abs"].max() > 0, ref


def test_models_across_the_frame_edges_and_wholly_outside(ft):
    v, t, B, frames, K, inst, who, want = scene("257", 1, 96, 96, per_subject=6)
    f = float(K[0, 0])
    for i, (dx, dy) in enumerate([(-48, 0), (48, 0), (0, -48), (0, 48), (4000, 0), (0, -4000)]):   # pixels, at the pose's depth
        z = float(inst[i]["t"][2])
        inst[i]["t"] = inst[i]["t"] + np.array([dx * z / f, dy * z / f, 0.0], np.float32)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 1, max_offset=16.0) as got:
        ref = step_both(ft, got, want, frames, K, inst, who, SMALL, "edges")
        assert ref["instances"][0] < 6


@pytest.mark.parametrize("prm_kw", [dict(iterations=0), dict(iterations=1), dict(iterations=32), dict(iterations=256), dict(mu=0.0), dict(min_count=1),
                                    dict(min_count=5), dict(min_cos2=0.0), dict(min_cos2=0.9), dict(eps=1e-6, mu=3.0), dict(gate=4.0)],
                         ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_the_parameters(ft, prm_kw):
    v, t, B, frames, K, inst, who, want = scene("162", 3, 160, 120, per_subject=6)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3, max_offset=16.0) as got:
        ref = step_both(ft, got, want, frames, K, inst, who, dict(SMALL, **prm_kw), str(prm_kw), device=True)
        if prm_kw.get("iterations") == 0:
            assert not want.offsets.any() and (ref["max_abs"] == 0).all()


def test_a_step_that_clamps_few_points_and_two_consecutive_steps(ft):
    v, t, B, frames, K, inst, who, want = scene("162", 3, 160, 120, per_subject=6, max_offset=0.75)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3, max_offset=0.75) as got:
        ref = step_both(ft, got, want, frames, K, inst, who, SMALL, "clamp")
        assert (ref["clamped"] > 0).all() and (ref["max_abs"] == 0.75).all()
        before = want.offsets.copy()
        ref = step_both(ft, got, want, frames, K, inst, who, dict(min_points=30000), "few points")
        assert (ref["status"] == su.FEW_POINTS).all() and (want.offsets == before).all() and (ref["points"] > 0).all()
    v, t, B, frames, K, inst, who, want = scene("162", 3, 160, 120, per_subject=6)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3, max_offset=16.0) as got:
        step_both(ft, got, want, frames, K, inst, who, SMALL, "first")
        first = want.offsets.copy()
        step_both(ft, got, want, frames, K, inst, who, SMALL, "second", device=True)
        assert (want.offsets != first).any()


def test_instances_that_take_no_part(ft):
    """A fit record that is not OK, a skipped instance, fewer subjects than the set (an instance of the subject left out is
    skipped by the device), a frame that does not exist (the _device form), and no instances at all."""
    v, t, B, frames, K, inst, who, want = scene("162", 3, 160, 120, per_subject=4)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3, max_offset=16.0) as got:
        status = np.zeros(len(inst), np.uint32)
        status[[1, 6]] = (fr.FEW_POINTS, fr.SINGULAR)
        skip = who.copy()
        skip[[2, 9]] = 0xFFFFFFFF
        ref = step_both(ft, got, want, frames, K, inst, skip, SMALL, "not ok, skipped", fit_status=status)
        assert ref["instances"].tolist() == [2, 3, 3]
        two = step_both(ft, got, want, frames, K, inst, who, SMALL, "two of three subjects", n_subjects=2, device=True)
        assert len(two) == 2 and two["instances"].tolist() == [4, 4]
        bad = [dict(i) for i in inst]
        bad[0]["frame"] = 99
        ref = step_both(ft, got, want, frames, K, bad, who, SMALL, "a frame that does not exist", device=True)
        assert ref["instances"][0] == 3
        # what the host forms refuse per instance, the device skips: a NaN in t, an infinite R, an R that is no rotation, a scale
        # that carries the set's bound past the extent limit
        bad = [dict(i) for i in inst]
        bad[0]["t"] = np.array([np.nan, 0.0, 800.0], np.float32)
        bad[1]["R"] = np.where(np.eye(3, dtype=bool), np.float32(np.inf), inst[1]["R"])
        bad[4]["R"] = (inst[4]["R"] * np.float32(1.02)).astype(np.float32)          # R R^T = 1.0404 I: 0.0404 above the tolerance of 0.02
        bad[5]["R"] = (inst[5]["R"] * np.float32(1.005)).astype(np.float32)         # 1.010025 I: within it, takes part
        bad[8]["scale"] = np.float32(40.0)                                          # 40 * the bound (about 150 mm) > 4096
        ref = step_both(ft, got, want, frames, K, bad, who, SMALL, "faulty instances", device=True)
        assert ref["instances"].tolist() == [2, 3, 3], ref
        for host_bad, text in ((0, "non-finite"), (4, "instance 4"), (8, "spans")):
            only = [dict(i) for i in inst]
            only[host_bad] = bad[host_bad]
            with pytest.raises(_lib.DepthheadError, match=text):
                ft.surface_step_subjects(frames, got, records(only), K, subjects=who)
        same(got, want, "refused by the host form")
        before = want.offsets.copy()
        for device in (False, True):
            ref = step_both(ft, got, want, frames, K, [], who[:0], SMALL, "no instances", device=device)
            assert (ref["status"] == su.FEW_POINTS).all() and (ref["points"] == 0).all() and (want.offsets == before).all()


def test_host_form_against_the_device_form_after_a_device_fit_between_guard_bands(ft):
    """The _device form on a side stream, fed by a device fit's instances and records, its records written between guard bands;
    the host form on a second set from the same fit read back: both equal the restatement."""
    import torch
    v, t, B, frames, K, inst, who, want = scene("162", 3, 160, 120, per_subject=3)
    rough = [dict(i, t=i["t"] + np.array([3.0, -2.0, 4.0], np.float32)) for i in inst]
    lib = _lib.load()
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3, max_offset=16.0) as got, fit.Subjects(v, t, basis, 3, max_offset=16.0) as host:
        start = records(rough)
        start["mesh"] = who
        stream = torch.cuda.Stream()
        band = 256
        out = torch.full((2 * band + 3 * REC.itemsize,), 0xCD, dtype=torch.uint8, device="cuda")
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_who = torch.from_numpy(who.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        Kf = np.ascontiguousarray(K, np.float32).reshape(9)
        with torch.cuda.stream(stream):
            d_inst, d_frec = ft.fit(d_frames, got.models, start, K, device_out=True, stream=stream.cuda_stream)
            fit.check(lib.dh_fit_surface_subjects_device(ft._h, C.c_void_p(d_frames.data_ptr()), len(frames), 160, 120, _lib.vp(Kf), got._h,
                                                         C.c_void_p(d_inst.data_ptr()), C.c_uint32(len(inst)), C.c_void_p(d_who.data_ptr()), C.c_uint32(3),
                                                         C.c_void_p(d_frec.data_ptr()), None, C.c_void_p(out.data_ptr() + band), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        raw = out.cpu().numpy()
        assert (raw[:band] == 0xCD).all() and (raw[-band:] == 0xCD).all()
        fitted, frec = d_inst.cpu().numpy().view(INST), d_frec.cpu().numpy().view(FREC)
        ref_inst = [us.instance(int(r["frame"]), r["R"].reshape(3, 3), r["t"], r["scale"]) for r in fitted]
        ref = su.surface_step(frames, K, want, ref_inst, who, 3, frec["status"], su.params())
        assert raw[band:-band].tobytes() == ref.tobytes()
        same(got, want, "device form")
        rec = ft.surface_step_subjects(frames, host, fitted, K, subjects=who, fit_records=frec)
        assert rec.tobytes() == ref.tobytes()
        same(host, want, "host form")


def test_the_camera_twins_with_a_matrix_that_is_no_pinhole(ft):
    from depthhead_amd import tracking
    v, t, B, frames, K, inst, who, want = scene("162", 3, 160, 120, per_subject=2)
    Ks = np.tile(np.asarray(K, np.float32), (len(frames), 1, 1))
    Ks[:, 0, 1] = 3.0                                      # a skew
    Ks[:, 2, 0] = 1e-5                                     # and a last row that is not (0, 0, 1)
    Ks[1::2, 0, 2] += 5.0
    import torch
    with tracking.Cameras(Ks) as cams, fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3, max_offset=16.0) as got, \
            fit.Subjects(v, t, basis, 3, max_offset=16.0) as dev:
        rec = ft.surface_step_subjects(frames, got, records(inst), cams, subjects=who, params=fit.surface_params(**SMALL))
        d_rec = ft.surface_step_subjects(torch.from_numpy(frames.view(np.int16).copy()).cuda(), dev, to_device(records(inst)), cams,
                                         subjects=torch.from_numpy(who.view(np.int32).copy()).cuda(), params=fit.surface_params(**SMALL), device_out=True)
        torch.cuda.synchronize()
        ref = su.surface_step(frames, Ks, want, inst, who, 3, None, su.params(**SMALL))
        assert rec.tobytes() == ref.tobytes() == d_rec.cpu().numpy().tobytes()
        same(got, want, "cameras")
        same(dev, want, "cameras, device")


def test_set_offsets_round_trip_and_a_refined_model_through_the_fit_and_the_shape_step(ft):
    """set_offsets / offsets; then Fitter.fit and shape_step_subjects with the refined models give the bytes they give with fresh
    models built on the host from the same points and normals."""
    v, t, B, frames, K, inst, who, want = scene("162", 3, 160, 120, per_subject=3)
    o = [np.clip(displacement(v, 50 + s), -16, 16) for s in range(3)]
    o[2][:] = np.where(np.arange(len(v)) % 2 == 0, 16.0, -16.0)                     # at the limits
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3, max_offset=16.0) as got:
        for s in range(3):
            got.set_offsets(s, o[s])
            want.set_offsets(s, o[s])
            assert got.offsets(s).tobytes() == np.asarray(o[s], np.float64).tobytes()
        same(got, want, "set_offsets")
        start = records(inst)
        start["mesh"] = who
        fitted, frec = ft.fit(frames, got.models, start, K)
        fresh = [fit.Model(want.pts[s], want.nrm[s]) for s in range(3)]
        try:
            fitted2, frec2 = ft.fit(frames, fresh, start, K)
            assert fitted.tobytes() == fitted2.tobytes() and frec.tobytes() == frec2.tobytes() and (frec["status"] == fit.FIT_OK).any()
            srec = ft.shape_step_subjects(frames, got, fitted, K, subjects=who, fit_records=frec, params=fit.shape_params(min_points=1))
            for s in range(3):
                one = np.where(who == s, 0, 0xFFFFFFFF).astype(np.uint32)
                one[frec["status"] != fit.FIT_OK] = 0xFFFFFFFF
                alone = ft.shape_step(frames, fresh[s], basis, fitted, K, subjects=one, params=fit.shape_params(min_points=1))[0]
                assert srec[s].tobytes() == alone.tobytes(), s
        finally:
            for m in fresh:
                m.close()


def test_an_ordinary_set_keeps_its_bytes_and_refuses_the_surface_calls(ft):
    v, t, B, frames, K, inst, who, want = scene("162", 3, 160, 120, per_subject=2)
    plain_ref = sb.Set(v, t, B, 3)
    lib = _lib.load()
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3) as plain, fit.Subjects(v, t, basis, 3, max_offset=16.0) as got:
        c = np.array([[0.2], [-0.1], [0.0]])
        plain.set_coeffs(c)
        plain_ref.set_coeffs(c)
        before = [plain.read(s) for s in range(3)]
        step_both(ft, got, want, frames, K, inst, who, SMALL, "the other set")
        assert plain.info()[4] == float(plain_ref.radius)
        for s in range(3):
            pts, nrm = plain.read(s)
            assert pts.tobytes() == before[s][0].tobytes() == plain_ref.pts[s].tobytes() and nrm.tobytes() == before[s][1].tobytes() == plain_ref.nrm[s].tobytes()
        assert plain.state().tobytes() == plain_ref.state.tobytes()
        # the surface calls on the ordinary set
        buf = np.full(len(v), 0.0)
        for call in (lambda: plain.set_offsets(0, buf), lambda: plain.offsets(0),
                     lambda: ft.surface_step_subjects(frames, plain, records(inst), K, subjects=who)):
            with pytest.raises(_lib.DepthheadError, match="holds no offsets"):
                call()
        # the refusals that need a real surface set, outputs untouched
        rec = np.full(3 * REC.itemsize, 0xCD, np.uint8)
        Kf, fr16, ri = np.ascontiguousarray(K, np.float32).reshape(9), np.ascontiguousarray(frames), records(inst)

        def call(n_subjects=3, prm=None, instances=ri, n_inst=None, subjects=who):
            rc = lib.dh_fit_surface_subjects(ft._h, _lib.vp(fr16), len(frames), 160, 120, _lib.vp(Kf), got._h, _lib.vp(instances),
                                             C.c_uint32(len(instances) if n_inst is None else n_inst), _lib.vp(subjects), C.c_uint32(n_subjects), None,
                                             C.byref(prm) if prm is not None else None, _lib.vp(rec))
            assert rc == EINVAL and (rec == 0xCD).all()
            return lib.dh_last_error().decode()

        assert "n_subjects = 4" in call(n_subjects=4) and "n_subjects = 0" in call(n_subjects=0)
        for kw, text in ((dict(gate=np.nan), "not finite"), (dict(eps=np.inf), "not finite"), (dict(gate=300.0), "gate"), (dict(gate=0.0), "gate"),
                         (dict(min_cos2=1.5), "min_cos2"), (dict(min_cos2=-0.1), "min_cos2"), (dict(mu=-1.0), "mu"), (dict(eps=0.0), "eps"),
                         (dict(min_count=0), "min_count"), (dict(min_points=0), "min_points"), (dict(iterations=257), "iterations")):
            assert text in call(prm=fit.surface_params(**kw)), kw
        p = fit.surface_params()
        p.reserved0 = 1
        assert "reserved" in call(prm=p)
        assert "NULL instances" in call(instances=None, n_inst=2)
        bad = ri.copy(); bad["scale"][1] = 65.0
        assert "instance 1 spans" in call(instances=bad)                        # (section 18's extent refusal comes first)
        bad = ri.copy(); bad["frame"][2] = 77
        assert "instance 2 names frame 77" in call(instances=bad)
        odd = who.copy(); odd[3] = 5
        assert "instance 3 names subject 5" in call(subjects=odd)
        for x in (np.nan, 16.5, -np.inf):
            o = np.zeros(len(v)); o[7] = x
            with pytest.raises(_lib.DepthheadError, match="offset 7"):
                got.set_offsets(1, o)
        with pytest.raises(_lib.DepthheadError, match="subject 3 of 3"):
            got.offsets(3)
        same(got, want, "after the refusals")
    with fit.ShapeBasis(B) as basis:
        with pytest.raises(_lib.DepthheadError, match="max_offset"):
            fit.Subjects(v, t, basis, 3, max_offset=64.5)
    # a model small enough for a scale beyond DH_SURFACE_MAX_SCALE to pass the extent test: the host form refuses it, the device skips it
    v, t, B, frames, K, inst, who, want = scene("4", 1, 96, 96, per_subject=3, max_offset=1.0)
    inst[1]["scale"] = np.float32(64.5)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 1, max_offset=1.0) as got:
        with pytest.raises(_lib.DepthheadError, match=r"instance 1 has \|scale\| = 64.5 above 64"):
            ft.surface_step_subjects(frames, got, records(inst), K, subjects=who)
        same(got, want, "refused")
        ref = step_both(ft, got, want, frames, K, inst, who, SMALL, "a scale the device skips", device=True)
        assert ref["instances"][0] <= 2


def test_refine_subjects_against_the_restated_driver_and_two_runs(ft):
    """fit.refine_subjects at S = 3, two rounds, the first with a shape step -- against surface_ref.refine_subjects; a second run
    from a fresh set gives the same bytes."""
    v, t, _, B = ss.generic()
    frames, K, starts, who = sc.three_subjects()
    use = [i for i in range(len(starts)) if starts[i]["frame"] % 8 < 3]             # three poses a subject
    starts, who = [starts[i] for i in use], [who[i] for i in use]
    want = su.Set(v, t, B, 3, max_offset=16.0)
    state, inst, (frec, urec), _ = su.refine_subjects(frames, K, want, starts, who, rounds=2, shape_rounds=1)
    runs = []
    for _ in range(2):
        with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3, max_offset=16.0) as got:
            g_state, g_inst, (g_frec, g_urec) = fit.refine_subjects(ft, frames, K, got, ss.as_records(starts), who, rounds=2, shape_rounds=1)
            same(got, want, "refined")
            runs.append((g_state.tobytes(), g_inst.tobytes(), g_frec.tobytes(), g_urec.tobytes(), got.offsets(1).tobytes(), got.read(2)[0].tobytes()))
            assert g_urec.tobytes() == urec.tobytes() and g_state.tobytes() == state.tobytes()
            assert [int(r["status"]) for r in frec] == g_frec["status"].tolist() and [int(r["points"]) for r in frec] == g_frec["points"].tolist()
            for a, b in zip(g_inst, inst):
                assert a["R"].tobytes() == np.asarray(b["R"], np.float32).tobytes() and a["t"].tobytes() == np.asarray(b["t"], np.float32).tobytes()
    assert runs[0] == runs[1]
