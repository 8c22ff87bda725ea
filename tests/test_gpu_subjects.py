"""A shape per subject on the GPU (k_subjects.hip) against its restatement tests/subjects_ref.py: every point,
normal, state and record equal, with no tolerance.  The update's normals are also the measurement of the device's f64 square
root against numpy's (test_the_square_root_is_numpys).  Scenes are those of tests/subjects_scenes.py and tests/shape_scenes.py;
frames are 160x120, models head_mesh(2) except where a size is the point."""
import ctypes as C
import functools

import numpy as np
import pytest

import shape_ref as sr
import shape_scenes as ss
import subjects_ref as sb
import subjects_scenes as sc
from gpu_kit import to_device
from depthhead_amd import _lib, fit, synth

pytestmark = pytest.mark.gpu

INST, REC, FREC, STATE = _lib.RENDER_INSTANCE_DTYPE, _lib.SHAPE_RECORD_DTYPE, _lib.FIT_RECORD_DTYPE, _lib.SUBJECT_STATE_DTYPE
W, H = sc.W, sc.H


@functools.lru_cache(maxsize=None)
def meshes():
    """name -> (verts, tris, eight seeded fields): 4, 255, 256, 257 and 2562 vertices -- either side of the update's 256 lanes, more
    than one workgroup a subject -- and the fan whose hub lies in 300 triangles."""
    tetra = (np.array([(0, 0, 0), (40, 0, 0), (0, 40, 0), (0, 0, 40)], np.float32), np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.uint32))
    out = {"4": tetra, "255": sc.lathe_mesh(11, 23), "256": sc.lathe_mesh(2, 127), "257": sc.lathe_mesh(15, 17), "2562": synth.head_mesh(4),
           "fan": sc.fan_mesh()}
    assert [len(out[k][0]) for k in ("4", "255", "256", "257", "2562", "fan")] == [4, 255, 256, 257, 2562, 301]
    return {k: (v, t, sc.seeded_fields(v, 8, 500 + i)) for i, (k, (v, t)) in enumerate(out.items())}


def coeff_sets(n_subjects, nk, seed):
    """[S, K] coefficients in [-0.5, 0.5]: seeded, the first subject's all 0, the last one's at the limits."""
    c = synth.SplitMix(seed).uniform(n_subjects * nk).reshape(n_subjects, nk) - 0.5
    c[0] = 0.0
    if n_subjects > 1:
        c[-1] = np.where(np.arange(nk) % 2 == 0, 0.5, -0.5)
    return c


def same_set(got, want, what):
    """The set on the GPU (a fit.Subjects) against the restated one: every state, point and normal."""
    state = got.state()
    assert state.dtype == STATE and state.tobytes() == want.state.tobytes(), (what, state, want.state)
    for s in range(len(want)):
        pts, nrm = got.read(s)
        assert pts.tobytes() == want.pts[s].tobytes(), (what, "points", s, int((pts != want.pts[s]).sum()))
        assert nrm.tobytes() == want.nrm[s].tobytes(), (what, "normals", s, int((nrm != want.nrm[s]).sum()))


def records(deltas, statuses=None):
    rec = np.zeros(len(deltas), REC)
    for i, d in enumerate(deltas):
        rec["delta"][i, :len(d)] = d
    rec["status"] = sr.OK if statuses is None else statuses
    rec["points"], rec["instances"], rec["sum_r2_fixed"] = 1000, 8, 123456        # what an update does not read
    return rec


CASES = [("4", 4, 3), ("255", 4, 3), ("256", 4, 3), ("257", 4, 3), ("2562", 4, 3), ("fan", 4, 3), ("257", 1, 1), ("257", 8, 1), ("257", 1, 65),
         ("257", 8, 65), ("256", 1, 3), ("255", 8, 3)]


@pytest.mark.parametrize("name,nk,n_subjects", CASES)
def test_points_normals_and_state_after_an_update(name, nk, n_subjects):
    """At creation (all coefficients 0), after set_coeffs, and after one update -- the host form where S is odd, the _device form
    on a side stream elsewhere -- whose increments push some coefficients through the clamp."""
    import torch
    v, t, B = meshes()[name]
    B = B[:nk]
    want = sb.Set(v, t, B, n_subjects)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, n_subjects) as got:
        assert got.info() == (len(v), len(t), nk, n_subjects, float(want.radius), 0)
        assert [m.info() for m in got.models] == [(len(v), float(want.radius))] * n_subjects
        same_set(got, want, "created")
        c = coeff_sets(n_subjects, nk, 900 + nk)
        got.set_coeffs(c)
        want.set_coeffs(c)
        same_set(got, want, "set_coeffs")
        delta = 0.6 * (synth.SplitMix(77 + n_subjects).uniform(n_subjects * nk).reshape(n_subjects, nk) - 0.5)
        if n_subjects > 1:
            delta[-1] = 0.3 * np.sign(c[-1])                                # the last subject stands at the limits: every field is clamped
        rec = records(delta)
        if n_subjects % 2:
            got.update(rec)
        else:
            stream = torch.cuda.Stream()
            d_rec = to_device(rec)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                got.update(d_rec, device=True, stream=stream.cuda_stream)
            stream.synchronize()
        want.update(rec)
        same_set(got, want, "update")
        assert (want.state["applied"] == 1).all() and (n_subjects == 1 or want.state["flags"][-1] == sb.CLAMPED)


def test_the_square_root_is_numpys():
    """The one operation the fit family had not run on the device: 27 coefficient sets of the 2562-point head, 69 174 normals,
    each the device's sqrt(q) against numpy's correctly rounded one through n / ln rounded to f32 -- and the states, whose
    zero_normals come from `ln > 0`.  The count of differing normals is printed before it is asserted to be 0."""
    v, t, B = meshes()["2562"]
    differing = total = 0
    with fit.ShapeBasis(B[:4]) as basis, fit.Subjects(v, t, basis, 9) as got:
        want = sb.Set(v, t, B[:4], 9)
        for seed in (1, 2, 3):
            c = coeff_sets(9, 4, seed)
            got.set_coeffs(c)
            want.set_coeffs(c)
            for s in range(9):
                pts, nrm = got.read(s)
                assert pts.tobytes() == want.pts[s].tobytes()
                differing += int((nrm.view(np.uint32) != want.nrm[s].view(np.uint32)).any(axis=1).sum())
                total += len(nrm)
            assert got.state().tobytes() == want.state.tobytes()
    print(f"square root: {differing} of {total} normals differ from numpy's")
    assert total >= 20000 and differing == 0


def test_clamped_non_finite_and_not_ok_records():
    """Eight subjects, one record each: an ordinary increment, one through +max_coeff and one through -max_coeff, a NaN, both
    infinities, DH_SHAPE_FEW_POINTS and DH_SHAPE_SINGULAR (whose deltas are not read).  Applied twice -- the host form, then the
    _device form -- so that the counters and the flags that stay are seen."""
    v, t, B = meshes()["257"]
    rec = records([(0.1, -0.1, 0.05, 0.0), (0.4, 0.0, 0.0, 0.0), (0.0, -0.4, 0.0, 0.0), (0.1, np.nan, 0.1, 0.1), (np.inf, 0.1, 0.1, 0.1),
                   (0.1, 0.1, 0.1, -np.inf), (0.3, 0.3, 0.3, 0.3), (np.nan, 0.3, 0.3, 0.3)],
                  [sr.OK] * 6 + [sr.FEW_POINTS, sr.SINGULAR])
    want = sb.Set(v, t, B[:4], 8)
    with fit.ShapeBasis(B[:4]) as basis, fit.Subjects(v, t, basis, 8) as got:
        start = np.tile(np.array([0.2, -0.2, 0.0, 0.1]), (8, 1))
        got.set_coeffs(start)
        want.set_coeffs(start)
        got.update(rec)
        want.update(rec)
        same_set(got, want, "host update")
        assert want.state["applied"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and want.state["rejected"].tolist() == [0, 0, 0, 1, 1, 1, 0, 0]
        assert want.state["flags"].tolist() == [0, sb.CLAMPED, sb.CLAMPED, sb.NONFINITE, sb.NONFINITE, sb.NONFINITE, 0, 0]
        assert want.state["coeffs"][1, 0] == 0.5 and want.state["coeffs"][2, 1] == -0.5 and want.state["coeffs"][6, :4].tolist() == [0.2, -0.2, 0.0, 0.1]
        import torch
        got.update(to_device(rec), device=True)
        torch.cuda.synchronize()
        want.update(rec)
        same_set(got, want, "device update")
        assert want.state["applied"].tolist() == [2, 2, 2, 0, 0, 0, 0, 0] and want.state["rejected"].tolist() == [0, 0, 0, 2, 2, 2, 0, 0]
        # set_coeffs clears the flags and keeps the counters
        got.set_coeffs(start[:2], first=3)
        want.set_coeffs(start[:2], first=3)
        same_set(got, want, "set_coeffs of two")
        assert want.state["flags"].tolist() == [0, sb.CLAMPED, sb.CLAMPED, 0, 0, sb.NONFINITE, 0, 0] and want.state["rejected"][3] == 2


def test_a_mesh_that_deforms_to_a_zero_normal():
    v, t, B, hub = sc.collapsing_disc()
    want = sb.Set(v, t, B, 3)
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3) as got:
        for c in ([[0.0], [0.25], [0.125]], [[0.25], [0.0], [0.25]]):
            got.set_coeffs(c)
            want.set_coeffs(c)
            same_set(got, want, "collapsed")
            assert want.state["zero_normals"].tolist() == [int(x[0] == 0.25) for x in c]
        assert not got.read(0)[1][hub].any() and got.read(1)[1][hub].any()
        # reached by an update as well: 0.125 + 0.125
        got.set_coeffs([[0.125]] * 3)
        want.set_coeffs([[0.125]] * 3)
        rec = records([(0.125,), (0.0,), (0.25,)])
        got.update(rec)
        want.update(rec)
        same_set(got, want, "collapsed by an update")
        assert want.state["zero_normals"].tolist() == [1, 0, 0]


@functools.lru_cache(maxsize=None)
def subject_frames():
    """(frames [8, H, W], K, the subject's eight true poses then its eight rough starts as records)"""
    frames, K, pos, Rs = ss.subject(W, H, 12)
    inst = ss.as_records(ss.true_instances(pos, Rs) + ss.rough_instances(12, pos, Rs))
    inst.setflags(write=False)
    return frames, K, inst


THREE = np.array(sc.VARIATIONS)


@pytest.fixture(scope="module")
def heads():
    """(fitter, basis, a set of three subjects of the generic head): the set's coefficients are whatever the last test left."""
    v, t, _, B = ss.generic()
    with fit.Fitter() as ft, fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, 3) as st:
        yield ft, basis, st


def test_models_of_a_set_through_the_fit(heads):
    """Fitter.fit with the set's models gives the bytes it gives with fresh models built on the host from the same coefficients,
    and an ordinary model fits to the same bytes before and after the set's calls."""
    ft, basis, st = heads
    v, t, n, B = ss.generic()
    frames, K, inst = subject_frames()
    starts = inst[8:].copy()
    with fit.Model(v, n) as plain:
        before = ft.fit(frames, [plain], starts, K)
        st.set_coeffs(THREE)
        starts["mesh"] = np.arange(8) % 3
        got = ft.fit(frames, st.models, starts, K)
        fresh = [fit.Model(fit.deform(v, B, c), fit.vertex_normals(fit.deform(v, B, c), t)) for c in THREE]
        want = ft.fit(frames, fresh, starts, K)
        for m in fresh:
            m.close()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert (got[1]["status"] == fit.FIT_OK).all()
        st.update(records([(0.01, 0.01, 0.01, 0.01)] * 3))
        starts["mesh"] = 0
        after = ft.fit(frames, [plain], starts, K)
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        # and the shape step of section 20 takes a model of the set as it takes any other
        st.set_coeffs(THREE)
        one = ft.shape_step(frames, st.models[1], basis, inst[:8], K)
        with fit.Model(*st.read(1)) as copy:
            assert one.tobytes() == ft.shape_step(frames, copy, basis, inst[:8], K).tobytes()


def restated(st_coeffs):
    v, t, _, B = ss.generic()
    want = sb.Set(v, t, B, len(st_coeffs))
    want.set_coeffs(st_coeffs)
    return want


def same_records(got, want, what):
    assert got.dtype == REC and want.dtype.itemsize == REC.itemsize
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), (what, i, got[i], want[i])
    assert got.tobytes() == want.tobytes(), what


def test_shape_step_subjects_against_the_restatement(heads):
    """Three subjects with different coefficients over sixteen instances: one whose fit record is not OK, one skipped by
    DH_SHAPE_SKIP, and both at once; then fewer subjects than the set has, no fit records, no subjects."""
    ft, basis, st = heads
    frames, K, inst = subject_frames()
    st.set_coeffs(THREE)
    want_set = restated(THREE)
    subjects = (np.arange(16) % 3).astype(np.uint32)
    subjects[7] = sr.SKIP
    subjects[9] = sr.SKIP
    frec = np.zeros(16, FREC)
    frec["points"], frec["steps"] = 100, 3
    frec["status"][[5, 9]] = (fit.FIT_FEW_POINTS, fit.FIT_SINGULAR)
    got = ft.shape_step_subjects(frames, st, inst, K, subjects=subjects, fit_records=frec)
    same_records(got, sb.shape_step(frames, K, want_set, inst, subjects, 3, frec["status"]), "three subjects")
    assert got["status"].tolist() == [fit.SHAPE_OK] * 3 and got["instances"].tolist() == [5, 4, 4]
    assert len({got[s].tobytes() for s in range(3)}) == 3
    # what a left-out instance holds changes nothing -- the host form refuses nothing about it
    junk = inst.copy()
    junk["frame"][5], junk["R"][5], junk["t"][9] = 4000, np.inf, np.nan
    same_records(ft.shape_step_subjects(frames, st, junk, K, subjects=subjects, fit_records=frec), got, "junk in the left out")
    two = ft.shape_step_subjects(frames, st, inst, K, subjects=np.where(subjects < 2, subjects, sr.SKIP), n_subjects=2)
    same_records(two, sb.shape_step(frames, K, want_set, inst, np.where(subjects < 2, subjects, sr.SKIP), 2), "two of three subjects")
    none = ft.shape_step_subjects(frames, st, inst, K)
    same_records(none, sb.shape_step(frames, K, want_set, inst, None, 3), "no subjects: all subject 0")
    assert none["instances"].tolist() == [16, 0, 0] and none["status"].tolist() == [fit.SHAPE_OK, fit.SHAPE_FEW_POINTS, fit.SHAPE_FEW_POINTS]
    empty = ft.shape_step_subjects(frames, st, inst[:0], K)
    assert empty["status"].tolist() == [fit.SHAPE_FEW_POINTS] * 3 and not empty["points"].any()


def test_shape_step_subjects_at_zero_coefficients_is_shape_step_on_the_base(heads):
    ft, basis, st = heads
    v, t, n, B = ss.generic()
    frames, K, inst = subject_frames()
    st.set_coeffs(np.zeros((3, 4)))
    subjects = (np.arange(16) % 3).astype(np.uint32)
    subjects[4] = sr.SKIP
    with fit.Model(v, n) as base:
        want = ft.shape_step(frames, base, basis, inst, K, subjects=subjects, n_subjects=3)
    same_records(ft.shape_step_subjects(frames, st, inst, K, subjects=subjects), want, "zero coefficients")
    same_records(want, sr.shape_step(frames, K, v, n, B, inst, subjects, 3), "and the restatement of section 20")


GUARD = 4096


def test_device_twins_on_a_side_stream_between_guard_bands(heads):
    """dh_fit_depth_device, then dh_fit_shape_subjects_device and its camera twin on the fit's outputs -- instances AND records --
    on a side stream with no host copy or wait between them; the shape records lie between 4 KB guard bands at a pointer 8 bytes
    off a 256-byte line.  Then an instance that names no frame, which the host form refuses and the device skips."""
    import torch
    from depthhead_amd.tracking import Cameras
    ft, basis, st = heads
    frames, K, inst = subject_frames()
    st.set_coeffs(THREE)
    want_set = restated(THREE)
    starts = inst[8:].copy()
    starts["mesh"] = np.arange(8) % 3
    starts["t"][6] += np.float32(400.0)                                    # a start the fit cannot recover: its record is not OK
    subjects = np.array([0, 1, 2, 0, 1, 2, 0, sr.SKIP], np.uint32)
    bytes_ = 3 * REC.itemsize
    stream = torch.cuda.Stream()
    with Cameras(np.tile(K.reshape(1, 9), (8, 1))) as cams:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_subj = torch.from_numpy(subjects.view(np.int32).copy()).cuda()
        bufs = [torch.full((GUARD + 8 + bytes_ + GUARD,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            d_out, d_frec = ft.fit(d_frames, st.models, starts, K, device_out=True, stream=stream.cuda_stream)
            for buf, kind, karg in ((bufs[0], "", _lib.vp(np.ascontiguousarray(K, np.float32).reshape(9))), (bufs[1], "_cameras", cams._h)):
                rc = getattr(ft._lib, "dh_fit_shape_subjects" + kind + "_device")(
                    ft._h, C.c_void_p(d_frames.data_ptr()), 8, W, H, karg, st._h, C.c_void_p(d_out.data_ptr()), C.c_uint32(8),
                    C.c_void_p(d_subj.data_ptr()), C.c_uint32(3), C.c_void_p(d_frec.data_ptr()), None, C.c_void_p(buf.data_ptr() + GUARD + 8),
                    C.c_void_p(stream.cuda_stream))
                _lib.check(rc)
        stream.synchronize()
        fitted = d_out.cpu().numpy().view(INST)
        frec = d_frec.cpu().numpy().view(FREC)
        assert frec["status"][6] != fit.FIT_OK and (np.delete(frec["status"], 6) == fit.FIT_OK).all()
        host = ft.shape_step_subjects(frames, st, fitted, K, subjects=subjects, fit_records=frec)
        want = sb.shape_step(frames, K, want_set, fitted, subjects, 3, frec["status"])
        same_records(host, want, "host form on the fitted instances")
        assert want["instances"].tolist() == [2, 2, 2]
        for buf in bufs:
            raw = buf.cpu().numpy()
            assert (raw[:GUARD + 8] == 0xEE).all() and (raw[GUARD + 8 + bytes_:] == 0xEE).all()
            same_records(raw[GUARD + 8:GUARD + 8 + bytes_].copy().view(REC), want, "device form")
        bad = fitted.copy()
        bad["frame"][2] = 999
        with pytest.raises(_lib.DepthheadError) as ei:
            ft.shape_step_subjects(frames, st, bad, K, subjects=subjects, fit_records=frec)
        assert ei.value.code == -1 and "names frame 999 of 8" in str(ei.value)
        got = ft.shape_step_subjects(d_frames, st, to_device(bad), K, subjects=d_subj, fit_records=d_frec, device_out=True)
        torch.cuda.synchronize()
        skipped = subjects.copy()
        skipped[2] = sr.SKIP
        same_records(got.cpu().numpy().view(REC), sb.shape_step(frames, K, want_set, fitted, skipped, 3, frec["status"]), "frame 999 skipped")


def test_a_carried_fit_starts_from_the_device_poses(heads):
    """fit(carried=) equals the host fit from the carried poses, keeps frame, mesh, scale and flags of the host instances, and
    falls back to the host instance's R and t where the carried ones are not finite or no rotation."""
    import torch
    ft, basis, st = heads
    frames, K, inst = subject_frames()
    st.set_coeffs(THREE)
    starts = inst[8:].copy()
    starts["mesh"], starts["flags"] = np.arange(8) % 3, 0x770000 + np.arange(8)
    prm = fit.fit_params(coarse_iterations=2, iterations=3)
    d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
    first, _ = ft.fit(d_frames, st.models, starts, K, params=prm, device_out=True)
    torch.cuda.synchronize()
    poses = first.cpu().numpy().view(INST).copy()
    want = ft.fit(frames, st.models, poses, K, params=prm)
    elsewhere = starts.copy()
    elsewhere["t"] += np.float32(50.0)                                    # what the carried poses replace
    got = ft.fit(d_frames, st.models, elsewhere, K, params=prm, device_out=True, carried=first)
    torch.cuda.synchronize()
    assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[1].cpu().numpy().tobytes() == want[1].tobytes()
    assert want[0]["flags"].tolist() == starts["flags"].tolist()
    uncarried = ft.fit(frames, st.models, elsewhere, K, params=prm)
    assert uncarried[0]["t"].tobytes() != want[0]["t"].tobytes()
    # carried poses the device does not take: instance 1 a NaN in t, 2 an infinite R, 3 an R that is no rotation, and a carried
    # frame, mesh and scale that are never read
    junk = poses.copy()
    junk["t"][1, 2], junk["R"][2, 4], junk["R"][3] = np.nan, np.inf, 1.5 * junk["R"][3]
    junk["frame"], junk["mesh"], junk["scale"] = 4000, 99, 1e30
    mixed = poses.copy()
    mixed[[1, 2, 3]] = starts[[1, 2, 3]]
    want = ft.fit(frames, st.models, mixed, K, params=prm)
    got = ft.fit(d_frames, st.models, starts, K, params=prm, device_out=True, carried=to_device(junk))
    torch.cuda.synchronize()
    assert got[0].cpu().numpy().tobytes() == want[0].tobytes() and got[1].cpu().numpy().tobytes() == want[1].tobytes()


def test_adapt_subjects_of_one_subject_is_adapt(heads):
    """S = 1: the coefficients, the instances and the last round's records of fit.adapt on the same inputs."""
    ft, basis, _ = heads
    v, t, _, B = ss.generic()
    frames, K, pos, Rs = ss.subject(W, H, 12)
    starts = ss.as_records(ss.rough_instances(12, pos, Rs))
    want_c, want_inst, trace = fit.adapt(ft, frames, K, v, t, B, starts)
    with fit.Subjects(v, t, basis, 1) as st:
        state, inst, (frec, srec) = fit.adapt_subjects(ft, frames, K, st, starts, np.zeros(8, np.uint32))
        assert state["coeffs"][0, :4].tobytes() == want_c.tobytes() and state["applied"][0] == 6 and state["flags"][0] == 0
        assert inst.tobytes() == want_inst.tobytes()
        assert frec.tobytes() == trace[-1]["fit"].tobytes() and srec[0].tobytes() == trace[-1]["shape"].tobytes()
        pts, nrm = st.read(0)
        assert pts.tobytes() == fit.deform(v, B, want_c).tobytes() and nrm.tobytes() == fit.vertex_normals(pts, t).tobytes()


def test_adapt_subjects_of_three_subjects_is_the_restatement_twice(heads):
    ft, basis, _ = heads
    v, t, _, B = ss.generic()
    frames, K, starts, who = sc.three_subjects()
    want_state, want_inst, (want_frec, want_srec), _ = sc.together()
    want_records = ss.as_records(want_inst)
    want_records["mesh"] = who
    runs = []
    for _ in range(2):
        with fit.Subjects(v, t, basis, 3) as st:
            state, inst, (frec, srec) = fit.adapt_subjects(ft, frames, K, st, ss.as_records(starts), who)
            runs.append(state.tobytes() + inst.tobytes() + frec.tobytes() + srec.tobytes() + b"".join(a.tobytes() for s in range(3) for a in st.read(s)))
    assert state.tobytes() == want_state.tobytes()
    assert inst.tobytes() == want_records.tobytes()
    want_fit = np.zeros(len(want_frec), FREC)                              # (the restated fit hands out dicts; `reserved` is 0)
    for i, r in enumerate(want_frec):
        want_fit[i] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"])
    assert frec.dtype == FREC and frec.tobytes() == want_fit.tobytes()
    same_records(srec, want_srec, "the last round's shape records")
    assert runs[0] == runs[1]


def test_refusals_that_need_a_device(heads):
    ft, basis, st = heads
    v, t, _, B = ss.generic()
    frames, K, inst = subject_frames()

    def refused(what, fn):
        with pytest.raises(_lib.DepthheadError) as ei:
            fn()
        assert ei.value.code == -1 and what in str(ei.value), str(ei.value)

    big_v, big_t, big_B = meshes()["257"]
    with fit.ShapeBasis(big_B[:2]) as other:
        refused("the basis is one of 257 points, the mesh has 162", lambda: fit.Subjects(v, t, other, 2))
    st.set_coeffs(THREE)
    before = st.state().tobytes() + b"".join(a.tobytes() for s in range(3) for a in st.read(s))
    refused("subject 3 of 3", lambda: _lib.check(st._lib.dh_fit_subjects_model(st._h, 3, C.byref(C.c_void_p()))))
    refused("subject 3 of 3", lambda: _lib.check(st._lib.dh_fit_subjects_read(st._h, 3, None, None)))
    refused("subjects 2 .. 4 of 3", lambda: st.set_coeffs(np.zeros((2, 4)), first=2))
    refused("NULL coefficients", lambda: _lib.check(st._lib.dh_fit_subjects_set_coeffs(st._h, 0, 1, None)))
    for bad in (np.nan, np.inf, -np.inf, np.nextafter(0.5, 1.0), -0.5000001):
        c = np.zeros((2, 4))
        c[1, 2] = bad
        refused("coefficient 2 of subject 2", lambda: st.set_coeffs(c, first=1))
    refused("NULL records", lambda: _lib.check(st._lib.dh_fit_subjects_update(st._h, None)))
    refused("NULL records", lambda: _lib.check(st._lib.dh_fit_subjects_update_device(st._h, None, None)))
    refused("NULL state", lambda: _lib.check(st._lib.dh_fit_subjects_state(st._h, None)))
    assert st.state().tobytes() + b"".join(a.tobytes() for s in range(3) for a in st.read(s)) == before
    st.set_coeffs(np.full((1, 4), 0.5), first=2)                            # the limit itself is a coefficient
    # the shape step: more subjects than the set holds, and the per-instance refusals with the SET'S BOUND for the radius
    refused("n_subjects = 4, expected 1 .. 3", lambda: ft.shape_step_subjects(frames, st, inst, K, n_subjects=4))
    refused("n_subjects = 0", lambda: ft.shape_step_subjects(frames, st, inst, K, n_subjects=0))
    refused("names subject 3 of 3", lambda: ft.shape_step_subjects(frames, st, inst, K, subjects=np.full(16, 3, np.uint32)))
    n, nt, nk, ns, bound, device = st.info()
    base_radius = float(np.sqrt((v.astype(np.float64) ** 2).sum(axis=1).max()))
    assert (n, nt, nk, ns, device) == (162, len(t), 4, 3, 0) and bound > base_radius * 1.5
    over = inst[:1].copy()
    over["scale"] = np.float32(4100.0 / bound)                              # within the extent by the base mesh, beyond it by the bound
    assert float(over["scale"][0]) * base_radius < 4096.0
    refused("spans", lambda: ft.shape_step_subjects(frames, st, over, K))
    refused("spans", lambda: ft.fit(frames, st.models, over, K))
    with fit.Model(v, fit.vertex_normals(v, t)) as plain:
        ft.fit(frames, [plain], over, K)                                    # (the base model alone is not refused)
