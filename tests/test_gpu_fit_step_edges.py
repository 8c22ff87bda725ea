"""The fit's step rule and the trackers' acceptance on the GPU, held to values placed on every compare (tests/fit_step_edges.py;
DESIGN.md section 18e).  The step cases -- a pivot of exactly 0.0 (in the fifth and in the last place), the smallest positive and
a negative one, x == 1e-6 and one step below it in the coarse and in the full phase, count == min_points and one more, a coarse
refusal that must keep the full phase from running -- go through every kernel that takes a step: k_fit (Fitter.fit, staged and
streamed), k_fit_sched (FitTracker.step_poses from a detected and from a carried start), k_fit_views (one identity view, and two
of which the second sees an empty frame), k_fit_views_sched (RigFitTracker.step_persons on a rig of one identity camera),
k_shape_solve and k_calib_solve; each in its host form and in its _device form.  The tracker cases -- the rms limit and
keep_points ON their compares, the jump test at d2 == jump2 and one f32 step beyond, the 96-bit validity compare in its high and
low words, the angle index and its clamps, lost == max_coast -- go through both trackers.  Every record is compared with the
hand-worked literals AND byte for byte with the restatement; nothing has a tolerance."""
import functools

import numpy as np
import pytest

import calib_ref as cr
import fit_edges as fe
import fit_ref as fr
import fit_step_edges as se
import fit_track_ref as tkr
import rig_fit_track_ref as rf
import shape_ref as sr
import view_fit_ref as vr
from gpu_kit import between_guards, to_device
from depthhead_amd import _lib, fit, tracking

pytestmark = pytest.mark.gpu

INST, REC, VINST, VREC = _lib.RENDER_INSTANCE_DTYPE, _lib.FIT_RECORD_DTYPE, _lib.VIEW_INSTANCE_DTYPE, _lib.VIEW_FIT_RECORD_DTYPE
TREC, RREC = _lib.FIT_TRACK_RECORD_DTYPE, _lib.RIG_FIT_RECORD_DTYPE
EYE = np.eye(3, dtype=np.float32)
GUARD = 4 * fe.W
FORMS = ("host", "device")
CASES = pytest.mark.parametrize("case", se.STEPS, ids=lambda c: c.name)
FULL_ONLY = pytest.mark.parametrize("case", [c for c in se.STEPS if c.coarse == 0], ids=lambda c: c.name)


class Bank:
    """The models on the GPU, made once."""

    def __init__(self):
        self.made = {}

    def get(self, key, pts, nrm):
        if key not in self.made:
            self.made[key] = fit.Model(pts, nrm)
        return self.made[key]

    def step(self, case, n):
        return self.get((case.name, n), *se.step_model(case, n))

    def close(self):
        for m in self.made.values():
            m.close()


@pytest.fixture(scope="module")
def gpu():
    bank = Bank()
    angles = fit.angles()
    angles.setflags(write=False)
    with fit.Fitter() as ft:
        yield ft, bank, angles
    bank.close()


def host(tensor, dtype):
    import torch
    torch.cuda.synchronize()
    return tensor.cpu().numpy().view(dtype)


def gpu_params(c, **kw):
    return fit.fit_params(**dict(dict(coarse_iterations=c.coarse, iterations=c.full, gate=c.gate, lam=c.lam, min_points=c.min_points), **kw))


def ref_params(c, **kw):
    return dict(fr.params(c.coarse, c.full, c.gate, c.lam, c.min_points), **kw)


def hold_step(case, rec, R, t, what):
    """A fit record and the fitted pose against the case's literals."""
    assert (rec["status"], rec["steps"], rec["reserved"]) == (case.status, case.steps, 0), (what, case.name, rec)
    if case.points is not None:
        assert rec["points"] == case.points, (what, case.name, rec)
    if case.e is not None:
        assert rec["sum_r2_fixed"] == case.e, (what, case.name, rec)
    if case.still:
        assert (np.asarray(R).reshape(3, 3) == EYE).all() and tuple(t) == case.t, (what, case.name, R, t)


@functools.lru_cache(maxsize=None)
def fit_restated(name, n):
    case = se.STEP_BY_NAME[name]
    pts, nrm = se.step_model(case, n)
    inst = se.step_instance(case)
    R, t, r = fr.fit(case.frame, fe.K, pts, nrm, EYE, case.t, 1.0, ref_params(case))
    out, rec = inst.copy(), np.zeros(1, REC)
    out[0]["R"], out[0]["t"] = R.reshape(9), t
    rec[0] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"])
    return out, rec


# ---------------------------------------------------------------- Fitter.fit: k_fit, staged and streamed
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", se.SIZES)
@CASES
def test_fit(gpu, case, n, form):
    ft, bank, _ = gpu
    model, inst = bank.step(case, n), se.step_instance(case)
    if form == "host":
        out, rec = ft.fit(case.frame[None], [model], inst, fe.K, params=gpu_params(case))
    else:
        frames, whole = between_guards(case.frame[None], GUARD, fe.BACK)
        out, rec = ft.fit(frames, [model], inst, fe.K, params=gpu_params(case), device_out=True)
        out, rec = host(out, INST), host(rec, REC)
    hold_step(case, rec[0], out[0]["R"], out[0]["t"], form)
    want_out, want_rec = fit_restated(case.name, n)
    assert rec.tobytes() == want_rec.tobytes() and out.tobytes() == want_out.tobytes(), (form, rec, want_rec, out, want_out)


# ---------------------------------------------------------------- Fitter.fit_views: k_fit_views
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("views", [0b01, 0b11])
@pytest.mark.parametrize("n", se.SIZES[1:])
@CASES
def test_fit_views(gpu, case, n, views, form):
    """One identity view; and two, of which the second sees an empty frame and adds nothing to any sum."""
    ft, bank, _ = gpu
    model = bank.step(case, n)
    frames = np.stack([case.frame, np.zeros_like(case.frame)])
    Ks = np.stack([fe.K, fe.K])
    inst = np.zeros(1, VINST)
    inst[0] = (0, 0, views, EYE.reshape(9), case.t, 1.0, 0x5E0000)
    with tracking.Cameras(Ks) as cams, fit.Views(cams, np.stack([EYE, EYE]), np.zeros((2, 3), np.float32)) as vw:
        if form == "host":
            out, rec = ft.fit_views(frames, [model], inst, vw, params=gpu_params(case))
        else:
            d_frames, whole = between_guards(frames, GUARD, fe.BACK)
            out, rec = ft.fit_views(d_frames, [model], inst, vw, params=gpu_params(case), device_out=True)
            out, rec = host(out, VINST), host(rec, VREC)
    hold_step(case, rec[0], out[0]["R"], out[0]["t"], form)
    R, t, r = vr.fit(frames, Ks, np.stack([EYE, EYE]), np.zeros((2, 3), np.float32), 0, views, *se.step_model(case, n), EYE, case.t, 1.0, ref_params(case))
    want = np.zeros(1, VREC)
    want[0] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"], r["views_used"])
    assert rec.tobytes() == want.tobytes(), (rec, want)
    assert out[0]["R"].tobytes() == R.tobytes() and out[0]["t"].tobytes() == t.tobytes()
    assert rec["views_used"][0] == (1 if rec["points"][0] else 0)
    _, plain = fit_restated(case.name, n)
    assert all(rec[f][0] == plain[f][0] for f in ("points", "steps", "status", "sum_r2_fixed"))


# ---------------------------------------------------------------- FitTracker.step_poses: k_fit_sched
def track_step(tracker, form, frames, poses, support, present=None, fit_params=None):
    """One core step of a FitTracker in its host form or in its _device form."""
    if form == "host":
        return tracker.step_poses(frames, poses, support, present=present, fit_params=fit_params)
    import torch
    d_frames, whole = between_guards(frames, GUARD, fe.BACK)
    d = [to_device(poses), to_device(support), to_device(np.asarray(present, np.uint8)) if present is not None else None]
    rec = torch.zeros(len(frames) * TREC.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tracker.step_device(d_frames.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), rec.data_ptr(), present_ptr=d[2].data_ptr() if d[2] is not None else 0,
                        fit_params=fit_params)
    return host(rec, TREC)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", se.SIZES[1:])
@CASES
def test_fit_tracker_from_a_detected_start(gpu, case, n, form):
    """A pose with rotation 0 and mid_point = the case's t: the start is R = I, t exactly, and the call's fit_params give the
    schedule.  The record's fit is the case's; the tracker believes every fit (a SINGULAR or FEW_POINTS one is REJECTED)."""
    ft, bank, angles = gpu
    model = bank.step(case, n)
    poses, support, kw = se.step_tracker_inputs(case)
    ref = tkr.Tracker(fe.K[None], *se.step_model(case, n), angles, prm=tkr.params(**kw))
    with tracking.Cameras(fe.K[None]) as cams, fit.FitTracker(cams, model, fe.W, fe.H, params=fit.fit_track_params(**kw)) as tracker:
        got = track_step(tracker, form, case.frame[None], poses, support, fit_params=gpu_params(case))
        want = ref.step(case.frame[None], poses, support, fit_prm=ref_params(case))
        rec = got[0]
        assert rec["status"] == (fit.FIT_TRACK_FITTED if case.status == se.OK else fit.FIT_TRACK_REJECTED | tkr.BAD_STATUS), rec
        if case.status == se.OK:
            hold_step(case, rec["fit"], rec["instance"]["R"], rec["instance"]["t"], form)
        else:
            hold_step(case._replace(still=False), rec["fit"], None, None, form)
            assert (rec["instance"]["R"].reshape(3, 3) == EYE).all() and tuple(rec["instance"]["t"]) == case.t
        assert got.tobytes() == want.tobytes(), (got, want)
        assert tracker.state().tobytes() == ref.state.tobytes()
        _, plain = fit_restated(case.name, n)
        assert rec["fit"].tobytes() == plain[0].tobytes()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", se.SIZES[1:])
@FULL_ONLY
def test_fit_tracker_from_a_carried_start(gpu, case, n, form):
    """Step 1 (schedule (0, 0)) is FITTED at the exact start and leaves R = I, t in the state; step 2 is carried and runs
    (0, iterations_tracked) with the case's lambda, gate and min_points from the call's fit_params."""
    ft, bank, angles = gpu
    model = bank.step(case, n)
    poses, support, kw = se.step_tracker_inputs(case)
    kw = dict(kw, iterations_tracked=case.full)
    ref = tkr.Tracker(fe.K[None], *se.step_model(case, n), angles, prm=tkr.params(**kw))
    with tracking.Cameras(fe.K[None]) as cams, fit.FitTracker(cams, model, fe.W, fe.H, params=fit.fit_track_params(**kw)) as tracker:
        first = track_step(tracker, form, case.frame[None], poses, support, fit_params=gpu_params(case, coarse_iterations=0, iterations=0))
        assert first[0]["status"] == fit.FIT_TRACK_FITTED and first[0]["fit"]["steps"] == 0
        assert first.tobytes() == ref.step(case.frame[None], poses, support, fit_prm=ref_params(case, coarse_iterations=0, iterations=0)).tobytes()
        got = track_step(tracker, form, case.frame[None], poses, support, fit_params=gpu_params(case, coarse_iterations=5))
        want = ref.step(case.frame[None], poses, support, fit_prm=ref_params(case, coarse_iterations=5))      # (a carried start has no coarse phase)
        rec = got[0]
        assert rec["status"] == (fit.FIT_TRACK_CARRIED if case.status == se.OK else fit.FIT_TRACK_REJECTED | tkr.BAD_STATUS), rec
        hold_step(case._replace(still=case.still and case.status == se.OK), rec["fit"], rec["instance"]["R"], rec["instance"]["t"], form)
        assert got.tobytes() == want.tobytes(), (got, want)
        assert tracker.state().tobytes() == ref.state.tobytes()
        _, plain = fit_restated(case.name, n)
        assert rec["fit"].tobytes() == plain[0].tobytes()


# ---------------------------------------------------------------- RigFitTracker.step_persons: k_fit_views_sched
class Rigged:
    """Cameras, rig table, identity view table and rig fit tracker of n_rigs rigs of `cams` cameras each, closed together."""

    def __init__(self, model, n_rigs, cams=1, **prm):
        n = n_rigs * cams
        self.Ks, self.V, self.u = np.stack([fe.K] * n), np.stack([EYE] * n), np.zeros((n, 3), np.float32)
        self.rig_begin = [g * cams for g in range(n_rigs + 1)]
        self.cams = tracking.Cameras(self.Ks)
        self.rig = tracking.Rig(self.cams, self.V, self.u, self.rig_begin)
        self.views = fit.Views(self.cams, self.V, self.u)
        self.tr = fit.RigFitTracker(self.rig, self.views, model, fe.W, fe.H, params=fit.rig_fit_track_params(**prm))

    def reference(self, pts, nrm, angles, **prm):
        return rf.Tracker(self.Ks, self.V, self.u, self.rig_begin, pts, nrm, angles, prm=rf.params(**prm))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in (self.tr, self.views, self.rig, self.cams):
            h.close()


def rig_step(tr, form, frames, inputs, present=None, fit_params=None):
    n_heads, heads, n_persons, persons = inputs
    if form == "host":
        return tr.step_persons(frames, n_heads, heads, n_persons, persons, present=present, fit_params=fit_params)
    import torch
    d_frames, whole = between_guards(frames, GUARD, fe.BACK)
    d = [to_device(a) for a in (n_heads, heads, n_persons, persons)]
    d_pr = to_device(np.asarray(present, np.uint8)) if present is not None else None
    rec = torch.zeros(len(n_persons) * 16 * RREC.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tr.step_device(d_frames.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), rec.data_ptr(), max_heads=heads.shape[1],
                   present_ptr=d_pr.data_ptr() if d_pr is not None else 0, fit_params=fit_params)
    return host(rec, RREC).reshape(len(n_persons), 16)


def rig_same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert len(got) == len(want) and got.dtype.itemsize == want.dtype.itemsize, what
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), (what, i, got[i], want[i])


def person_at(case):
    return se.rig_inputs(se._st(1, mid=[case.t]), _lib.RIG_PERSON_DTYPE, _lib.HEAD_DTYPE)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", se.SIZES[1:])
@CASES
def test_rig_fit_tracker_from_a_detected_start(gpu, case, n, form):
    """A rig of one identity camera: the person's world is the case's t and its head's rotation is 0, so the start is R = I, t."""
    ft, bank, angles = gpu
    model = bank.step(case, n)
    prm = {k: v for k, v in se.BELIEVE.items() if k != "min_windows"}
    with Rigged(model, 1, **prm) as rg:
        ref = rg.reference(*se.step_model(case, n), angles, **prm)
        got = rig_step(rg.tr, form, case.frame[None], person_at(case), fit_params=gpu_params(case))
        want = ref.step(case.frame[None], *person_at(case), fit_prm=ref_params(case))
        rec = got[0, 0]
        assert rec["status"] == (fit.FIT_TRACK_FITTED if case.status == se.OK else fit.FIT_TRACK_REJECTED | tkr.BAD_STATUS), rec
        hold_step(case._replace(still=case.still and case.status == se.OK), rec["fit"], rec["instance"]["R"], rec["instance"]["t"], form)
        rig_same(got, want, "records")
        rig_same(rg.tr.state(), ref.state, "state")
        _, plain = fit_restated(case.name, n)
        assert all(rec["fit"][f] == plain[f][0] for f in ("points", "steps", "status", "sum_r2_fixed"))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", se.SIZES[1:])
@FULL_ONLY
def test_rig_fit_tracker_from_a_carried_start(gpu, case, n, form):
    ft, bank, angles = gpu
    model = bank.step(case, n)
    prm = dict({k: v for k, v in se.BELIEVE.items() if k != "min_windows"}, iterations_tracked=case.full)
    with Rigged(model, 1, **prm) as rg:
        ref = rg.reference(*se.step_model(case, n), angles, **prm)
        first = rig_step(rg.tr, form, case.frame[None], person_at(case), fit_params=gpu_params(case, coarse_iterations=0, iterations=0))
        assert first[0, 0]["status"] == fit.FIT_TRACK_FITTED
        rig_same(first, ref.step(case.frame[None], *person_at(case), fit_prm=ref_params(case, coarse_iterations=0, iterations=0)), "first records")
        got = rig_step(rg.tr, form, case.frame[None], person_at(case), fit_params=gpu_params(case))
        want = ref.step(case.frame[None], *person_at(case), fit_prm=ref_params(case))
        rec = got[0, 0]
        assert rec["status"] == (fit.FIT_TRACK_CARRIED if case.status == se.OK else fit.FIT_TRACK_REJECTED | tkr.BAD_STATUS), rec
        hold_step(case._replace(still=case.still and case.status == se.OK), rec["fit"], rec["instance"]["R"], rec["instance"]["t"], form)
        rig_same(got, want, "records")
        rig_same(rg.tr.state(), ref.state, "state")


# ---------------------------------------------------------------- k_shape_solve and k_calib_solve
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", se.SHAPE_SIZES)
@pytest.mark.parametrize("case", se.SHAPES, ids=lambda c: c.name)
def test_shape_step_solve(gpu, case, n, form):
    ft, bank, _ = gpu
    pts, nrm, B = se.shape_model(n)
    model, inst = bank.get(("shape", n), pts, nrm), se.step_instance(se._SHAPE_CASE)
    prm = fit.shape_params(gate=25.0, lam=case.lam, min_points=case.min_points)
    with fit.ShapeBasis(B[:case.fields]) as basis:
        if form == "host":
            rec = ft.shape_step(se.F65[None], model, basis, inst, fe.K, params=prm)
        else:
            d_frames, whole = between_guards(se.F65[None], GUARD, fe.BACK)
            rec = host(ft.shape_step(d_frames, model, basis, to_device(inst), fe.K, params=prm, device_out=True), _lib.SHAPE_RECORD_DTYPE)
    got = (rec["status"][0], rec["points"][0], rec["sum_r2_fixed"][0], rec["instances"][0], rec["reserved"][0])
    assert got == (case.status, case.points, case.e, 1, 0), (case.name, got)
    if case.delta is not None:
        assert tuple(rec["delta"][0][:case.fields]) == case.delta and not rec["delta"][0][case.fields:].any()
    want = sr.shape_step(se.F65[None], fe.K, pts, nrm, B[:case.fields], inst, prm=sr.params(25.0, case.lam, case.min_points))
    assert rec.tobytes() == want.tobytes(), (rec, want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", se.SIZES[1:])
@pytest.mark.parametrize("case", se.CALIBS, ids=lambda c: c.name)
def test_calibrate_step_solve(gpu, case, n, form):
    ft, bank, _ = gpu
    model = bank.step(se.CALIB_CASE, n)
    frames = se.F65[None, None]
    inst = np.zeros(1, VINST)
    inst[0] = (0, 0, 1, EYE.reshape(9), fe.T, 1.0, 0)
    prm = fit.calib_params(gate=25.0, lam=0.0, min_points=case.min_points, pivot=fe.T)
    with tracking.Cameras(fe.K[None]) as cams, fit.Views(cams, EYE[None], np.zeros((1, 3), np.float32)) as vw:
        if form == "host":
            rec = ft.calibrate_step(frames, vw, model, inst, params=prm)
        else:
            d_frames, whole = between_guards(se.F65[None], GUARD, fe.BACK)
            rec = host(ft.calibrate_step(d_frames[None], vw, model, to_device(inst), params=prm, device_out=True), _lib.CALIB_RECORD_DTYPE)
    got = (rec["status"][0], rec["points"][0], rec["sum_r2_fixed"][0], rec["pairs"][0])
    assert got == (case.status, case.points, case.e, 1), (case.name, got)
    want = cr.calib_step(frames, fe.K[None], EYE[None], np.zeros((1, 3), np.float32), *se.step_model(se.CALIB_CASE, n), inst,
                         prm=cr.params(25.0, 0.0, case.min_points, fe.T))
    assert rec.tobytes() == want.tobytes(), (rec, want)


# ---------------------------------------------------------------- the trackers' rule
def script_frames(script, step, cams=1):
    tb = se.tracker_table(script.only)
    frame = np.zeros_like(tb.frames[0]) if step["empty"] else tb.frames[0]
    out = np.zeros((script.n, cams) + frame.shape, np.uint16)
    out[:, 0] = frame
    return tb, out.reshape((script.n * cams,) + frame.shape)


def hold_script(script, step, status, fit_rec, R, tracked, angles, what):
    for i, want in enumerate(step["want"]):
        assert status[i] == want, (what, script.name, i, hex(status[i]), hex(want))
        if want not in (se.NONE, se.ABSENT) and step["points"] is not None:
            got = (fit_rec["points"][i], fit_rec["sum_r2_fixed"][i], fit_rec["steps"][i], fit_rec["status"][i])
            assert got == (step["points"], step["e"], 0, se.OK), (what, script.name, i, got)
        if step["tracked"] is not None:
            assert tracked[i] == step["tracked"][i], (what, script.name, i)
    if script.name == "angles":
        for i, (name, rotation, index) in enumerate(se.ANGLES):
            middle = (index - 60 + 0.25) * se.BIN                  # a rotation in the middle of the entry's bin
            assert R[i].tobytes() == tkr.forest_rotation([middle] * 3, angles).tobytes(), (what, name)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("script", se.scripts(), ids=lambda s: s.name)
def test_fit_tracker_rule(gpu, script, form):
    ft, bank, angles = gpu
    tb = se.tracker_table(script.only)
    model = bank.get(("track", script.only), *tb.models[0])
    ref = tkr.Tracker(np.stack([fe.K] * script.n), *tb.models[0], angles, prm=tkr.params(**script.prm))
    prm, ref_prm = fit.fit_params(coarse_iterations=0, iterations=0, gate=(se.GATE, se.GATE)), fr.params(0, 0, (se.GATE, se.GATE))
    with tracking.Cameras(np.stack([fe.K] * script.n)) as cams, \
            fit.FitTracker(cams, model, fe.W, fe.H, params=fit.fit_track_params(**script.prm)) as tracker:
        for step in script.steps:
            _, frames = script_frames(script, step)
            poses, support = se.poses_of(step, _lib.POSE_DTYPE), se.support_of(step["support"])
            got = track_step(tracker, form, frames, poses, support, present=step["present"], fit_params=prm)
            want = ref.step(frames, poses, support, present=step["present"], fit_prm=ref_prm)
            state = tracker.state()
            hold_script(script, step, got["status"], got["fit"], got["instance"]["R"], state["tracked"], angles, form)
            assert got.tobytes() == want.tobytes(), (script.name, got, want)
            assert state.tobytes() == ref.state.tobytes(), script.name


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("script", se.scripts(rig=True), ids=lambda s: s.name)
def test_rig_fit_tracker_rule(gpu, script, form):
    """One rig of one identity camera per row, persons.world as the detection; the coast rows take a rig of two cameras, of which
    the one that saw the person is away in step 2."""
    ft, bank, angles = gpu
    tb = se.tracker_table(script.only)
    model = bank.get(("track", script.only), *tb.models[0])
    cams = 2 if script.name.startswith("coast") else 1
    kw = {k: v for k, v in script.prm.items() if k != "min_windows"}
    prm, ref_prm = fit.fit_params(coarse_iterations=0, iterations=0, gate=(se.GATE, se.GATE)), fr.params(0, 0, (se.GATE, se.GATE))
    with Rigged(model, script.n, cams, **kw) as rg:
        ref = rg.reference(*tb.models[0], angles, **kw)
        for k, step in enumerate(script.steps):
            _, frames = script_frames(script, step, cams)
            n_heads, heads, n_persons, persons = se.rig_inputs(step, _lib.RIG_PERSON_DTYPE, _lib.HEAD_DTYPE)
            if cams == 2:                               # heads [n_cams, 1]: the rig's second camera has none
                wide = np.zeros((2 * script.n, 1), _lib.HEAD_DTYPE)
                wide[::2], persons["best_cam"] = heads, persons["best_cam"] * 2
                heads, n_heads = wide, (np.repeat(n_heads, 2) * np.tile([1, 0], script.n)).astype(np.uint32)
            present = None if step["present"] is None else [0, 1] * script.n if cams == 2 else step["present"]
            got = rig_step(rg.tr, form, frames, (n_heads, heads, n_persons, persons), present=present, fit_params=prm)
            want = ref.step(frames, n_heads, heads, n_persons, persons, present=present, fit_prm=ref_prm)
            state = rg.tr.state()
            first = got[:, 0]
            hold_script(script, step, first["status"], first["fit"], first["instance"]["R"], state[:, 0]["tracked"], angles, form)
            rig_same(got, want, f"{script.name}: records of step {k}")
            rig_same(state, ref.state, f"{script.name}: state after step {k}")
            if k == 1:
                entry = state[0, 0]
                zero = not np.frombuffer(entry.tobytes(), np.uint8).any()
                if script.name in ("unseen_rejected_is_freed", "coast_above"):
                    assert zero, script.name
                if script.name == "seen_rejected_is_kept":
                    assert (entry["id"], entry["tracked"], entry["lost"]) == (7, 0, 1)
                if script.name == "coast_on":
                    assert (entry["id"], entry["tracked"], entry["lost"]) == (7, 1, 1)
