"""The fit family's point correspondence on the GPU, held to points placed on every compare (tests/fit_edges.py; DESIGN.md
section 18a).  The table -- one one-point model per row, and all rows in one model of 257 and of 1025 points at indices 0, 63, 64,
255, 256, 1023 and 1024 -- goes through every entry point that expands DH_FIT_CORRESPOND: Fitter.fit (one K, a camera table, the
_device twins, a carried start), FitTracker.step_poses (the one way into k_fit_sched), fit_views, shape_step, shape_step_views, shape_step_subjects, calibrate_step,
surface_step_subjects (with the grazing rows) and identify_subjects.  Every record is compared byte for byte with the
hand-worked literals AND with the restatement; no instance is left out and nothing has a tolerance.  In every _device form the
frames lie between guard bands of an in-gate depth, so that a read one element or one row past the last frame would keep the
corner row or y_equals_h.  The subject-set entry points take the aggregated models only (their normals come from a mesh).
Schedules are (0, 0): only the last pass runs and the pose comes back as it went in."""
import contextlib
import functools

import numpy as np
import pytest

import calib_ref as cr
import fit_edges as fe
import fit_ref as fr
import fit_track_ref as tkr
import ident_ref as ir
import shape_ref as sr
import shape_views_ref as svr
import subjects_ref as sb
import surface_ref as ur
import view_fit_ref as vr
from gpu_kit import between_guards, same_records, to_device
from depthhead_amd import _lib, fit
from depthhead_amd.tracking import Cameras

pytestmark = pytest.mark.gpu

INST, REC, VINST, VREC = _lib.RENDER_INSTANCE_DTYPE, _lib.FIT_RECORD_DTYPE, _lib.VIEW_INSTANCE_DTYPE, _lib.VIEW_FIT_RECORD_DTYPE
SREC, CREC, UREC = _lib.SHAPE_RECORD_DTYPE, _lib.CALIB_RECORD_DTYPE, _lib.SURFACE_RECORD_DTYPE
GUARD = 4 * fe.W                    # elements of an in-gate depth before and after the frames of a _device form
SIZES = (257, 1025)
EYE = np.eye(3, dtype=np.float32)
assert INST == fe.INST_DTYPE


class Bank:
    """The models on the GPU, made once: one per (row, mirrored) and one per aggregated model."""

    def __init__(self):
        self.made = {}

    def get(self, key, pts, nrm):
        if key not in self.made:
            self.made[key] = fit.Model(pts, nrm)
        return self.made[key]

    def rows(self, tb, mirrored):
        return [self.get((r.name, mirrored), *tb.models[i]) for i, r in enumerate(tb.rows)]

    def close(self):
        for m in self.made.values():
            m.close()


@pytest.fixture(scope="module")
def gpu():
    bank = Bank()
    with fit.Fitter() as ft:
        yield ft, bank
    bank.close()


@functools.lru_cache(maxsize=None)
def table(kind, gate, mirrored=False, own=True, pin=None):
    """kind: "rows" or the size of an aggregated model."""
    return fe.per_row(gate, mirrored, own) if kind == "rows" else fe.aggregated(kind, gate, mirrored, pin=pin)


def models_of(bank, kind, gate, mirrored, tb, pin=None):
    return bank.rows(tb, mirrored) if kind == "rows" else [bank.get((kind, gate, mirrored, pin), *tb.models[0])]


def literals(tb):
    p, e = (tb.points, tb.e) if isinstance(tb.points, list) else ([tb.points], [tb.e])
    return p, e, ([r.name for r in tb.rows] if isinstance(tb.points, list) else ["all rows"])


def host(tensor, dtype):
    import torch
    torch.cuda.synchronize()
    return tensor.cpu().numpy().view(dtype)


# ---------------------------------------------------------------- Fitter.fit
def fit_prm(gate, coarse=0, min_points=None):
    return fit.fit_params(coarse_iterations=coarse, iterations=0, gate=(gate, gate), min_points=min_points)


@functools.lru_cache(maxsize=None)
def fit_restated(kind, gate, mirrored, own, coarse=0):
    tb = table(kind, gate, mirrored, own)
    out, rec = tb.inst.copy(), np.zeros(len(tb.inst), REC)
    for i, it in enumerate(tb.inst):
        pts, nrm = tb.models[it["mesh"]]
        R, t, r = fr.fit(tb.frames[it["frame"]], tb.Ks[it["frame"]], pts, nrm, it["R"].reshape(3, 3), it["t"], it["scale"],
                         fr.params(coarse, 0, (gate, gate), min_points=6 if coarse else 16))
        out[i]["R"], out[i]["t"] = R.reshape(9), t
        rec[i] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"])
    return out, rec


def hold_fit(out, rec, tb, what):
    """The pose as it went in; points and sum_r2_fixed the literals; nothing else in the record."""
    points, e, names = literals(tb)
    assert out.tobytes() == tb.inst.tobytes(), what
    for i, name in enumerate(names):
        got = (rec["points"][i], rec["sum_r2_fixed"][i], rec["steps"][i], rec["status"][i], rec["reserved"][i])
        assert got == (points[i], e[i], 0, fit.FIT_OK, 0), (what, name, got, (points[i], e[i]))


FORMS = ("one_k", "cameras", "device", "cameras_device", "carried")


def run_fit(ft, ms, tb, gate, form, prm=None):
    prm = prm or fit_prm(gate)
    if form == "one_k":
        return ft.fit(tb.frames, ms, tb.inst, fe.K, params=prm)
    if form == "cameras":
        with Cameras(tb.Ks) as cams:
            return ft.fit(tb.frames, ms, tb.inst, cams, params=prm)
    frames, whole = between_guards(tb.frames, GUARD, fe.BACK)
    with Cameras(tb.Ks) as cams:
        if form == "carried":                          # the start comes from the carried poses, not from the instances
            off = tb.inst.copy()
            off["t"] += np.float32(3.0)
            out, rec = ft.fit(frames, ms, off, fe.K, params=prm, device_out=True, carried=to_device(tb.inst))
        else:
            out, rec = ft.fit(frames, ms, tb.inst, cams if form == "cameras_device" else fe.K, params=prm, device_out=True)
        return host(out, INST), host(rec, REC)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("gate", fe.GATES)
def test_fit_row_by_row(gpu, gate, mirrored, form):
    ft, bank = gpu
    own = form in ("cameras", "cameras_device")         # the rows with a K of their own need a camera table
    tb = table("rows", gate, mirrored, own)
    out, rec = run_fit(ft, bank.rows(tb, mirrored), tb, gate, form)
    hold_fit(out, rec, tb, form)
    want_out, want_rec = fit_restated("rows", gate, mirrored, own)
    same_records(rec, want_rec, "record"); same_records(out, want_out, "instance")


@pytest.mark.parametrize("form", ("cameras", "cameras_device"))
def test_fit_row_by_row_at_the_widest_gate(gpu, form):
    """gate = 4096, the fit's largest: the rows that belong to no gate, with the same literals (pixel_zero is still dropped by
    the pixel alone, pixel_65535 is kept one millimetre from its point)."""
    ft, bank = gpu
    tb = table("rows", 4096.0)
    assert len(tb.rows) == len(fe.ROWS) - 8 and "pixel_65535" in tb.index
    out, rec = run_fit(ft, bank.rows(tb, False), tb, 4096.0, form)
    hold_fit(out, rec, tb, form)
    want_out, want_rec = fit_restated("rows", 4096.0, False, True)
    same_records(rec, want_rec, "record"); same_records(out, want_out, "instance")


@pytest.mark.parametrize("form", ("one_k", "device", "carried"))
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gate", fe.GATES)
def test_fit_aggregated(gpu, gate, n, mirrored, form):
    ft, bank = gpu
    tb = table(n, gate, mirrored)
    ms = models_of(bank, n, gate, mirrored, tb)
    assert ms[0].info()[0] == n
    out, rec = run_fit(ft, ms, tb, gate, form)
    hold_fit(out, rec, tb, form)
    want_out, want_rec = fit_restated(n, gate, mirrored, True)
    same_records(rec, want_rec, "record"); same_records(out, want_out, "instance")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gate", fe.GATES)
def test_fit_aggregated_one_coarse_step_is_the_restated_one(gpu, gate, n):
    """Schedule (1, 0) with min_points = 6, the smallest the call takes (the table keeps 12 points): the coarse pass sees the edges
    too, then the pose moves; held to fit_ref alone."""
    ft, bank = gpu
    tb = table(n, gate)
    out, rec = run_fit(ft, models_of(bank, n, gate, False, tb), tb, gate, "one_k", fit_prm(gate, coarse=1, min_points=6))
    want_out, want_rec = fit_restated(n, gate, False, True, coarse=1)
    same_records(rec, want_rec, "record"); same_records(out, want_out, "instance")
    assert rec["steps"][0] == 1


# ---------------------------------------------------------------- FitTracker: the way into k_fit_sched
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gate", fe.GATES)
def test_fit_tracker_aggregated_from_the_forest_start_and_carried(gpu, gate, n, mirrored):
    """k_fit_sched, which only a FitTracker launches, on the table's exact start: a pose with rotation 0 (entry 60 of the angle
    table: R = I) and mid_point = T, schedule (0, 0).  The first step is FITTED from that start, the second CARRIED from the state,
    which holds the same R and t; both records carry the summed literals and equal fit_track_ref's byte for byte."""
    ft, bank = gpu
    tb = table(n, gate, mirrored)
    model = models_of(bank, n, gate, mirrored, tb)[0]
    poses, support, kw = fe.tracker_inputs()
    scale = float(tb.inst["scale"][0])
    ref = tkr.Tracker(tb.Ks, *tb.models[0], fit.angles(), scale=scale, prm=tkr.params(**kw))
    with Cameras(tb.Ks) as cams, fit.FitTracker(cams, model, fe.W, fe.H, scale=scale, params=fit.fit_track_params(**kw)) as tracker:
        for status in (fit.FIT_TRACK_FITTED, fit.FIT_TRACK_CARRIED):
            got = tracker.step_poses(tb.frames, poses, support, fit_params=fit_prm(gate))
            want = ref.step(tb.frames, poses, support, fit_prm=fr.params(0, 0, (gate, gate)))
            rec = got[0]
            seen = (rec["status"], rec["fit"]["points"], rec["fit"]["sum_r2_fixed"], rec["fit"]["steps"], rec["fit"]["status"])
            assert seen == (status, tb.points, tb.e, 0, fit.FIT_OK), seen
            assert (rec["instance"]["R"].reshape(3, 3) == EYE).all() and tuple(rec["instance"]["t"]) == fe.T
            assert got.tobytes() == want.tobytes(), (status, got, want)
            assert tracker.state().tobytes() == ref.state.tobytes(), status


# ---------------------------------------------------------------- Fitter.fit_views
def view_instances(inst, first_cam, views):
    out = np.zeros(len(inst), VINST)
    for i, it in enumerate(inst):
        out[i] = (first_cam[i], it["mesh"], views[i], it["R"], it["t"], it["scale"], it["flags"])
    return out


def views_restated(frames, Ks, inst, models, gate):
    n = len(frames)
    V, u = np.broadcast_to(EYE, (n, 3, 3)), np.zeros((n, 3), np.float32)
    rec = np.zeros(len(inst), VREC)
    for i, it in enumerate(inst):
        pts, nrm = models[it["model"]]
        R, t, r = vr.fit(frames, Ks, V, u, it["first_cam"], it["views"], pts, nrm, it["R"].reshape(3, 3), it["t"], it["scale"], fr.params(0, 0, (gate, gate)))
        assert R.tobytes() == it["R"].tobytes() and t.tobytes() == it["t"].tobytes()
        rec[i] = (r["points"], r["steps"], r["status"], 0, r["sum_r2_fixed"], r["views_used"])
    return rec


@contextlib.contextmanager
def identity_views(Ks):
    with Cameras(Ks) as cams, fit.Views(cams, np.broadcast_to(EYE, (len(Ks), 3, 3)), np.zeros((len(Ks), 3), np.float32)) as views:
        yield views


def run_views(ft, ms, frames, Ks, inst, gate, device):
    with identity_views(Ks) as views:
        if not device:
            return ft.fit_views(frames, ms, inst, views, params=fit_prm(gate))
        d_frames, whole = between_guards(frames, GUARD, fe.BACK)
        out, rec = ft.fit_views(d_frames, ms, inst, views, params=fit_prm(gate), device_out=True)
        return host(out, VINST), host(rec, VREC)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("gate", fe.GATES)
def test_fit_views_row_by_row_each_through_its_own_camera(gpu, gate, mirrored, device):
    """One identity view per row: instance i sees camera i alone (first_cam = i > 0 for all but the first)."""
    ft, bank = gpu
    tb = table("rows", gate, mirrored)
    inst = view_instances(tb.inst, range(len(tb.inst)), [1] * len(tb.inst))
    out, rec = run_views(ft, bank.rows(tb, mirrored), tb.frames, tb.Ks, inst, gate, device)
    assert out.tobytes() == inst.tobytes()
    for i, r in enumerate(tb.rows):
        got = (rec["points"][i], rec["sum_r2_fixed"][i], rec["views_used"][i], rec["steps"][i], rec["status"][i])
        assert got == (r.points, r.e, r.points, 0, fit.FIT_OK), (r.name, got)
    same_records(rec, views_restated(tb.frames, tb.Ks, inst, tb.models, gate), "record")


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gate", fe.GATES)
def test_fit_views_aggregated(gpu, gate, n, mirrored, device):
    ft, bank = gpu
    tb = table(n, gate, mirrored)
    inst = view_instances(tb.inst, [0], [1])
    out, rec = run_views(ft, models_of(bank, n, gate, mirrored, tb), tb.frames, tb.Ks, inst, gate, device)
    assert out.tobytes() == inst.tobytes()
    assert (rec["points"][0], rec["sum_r2_fixed"][0], rec["views_used"][0], rec["steps"][0]) == (tb.points, tb.e, 1, 0)
    same_records(rec, views_restated(tb.frames, tb.Ks, inst, tb.models, gate), "record")


@pytest.mark.parametrize("index", [0, 64, 128, 192, 256])
@pytest.mark.parametrize("name", ["x_zero", "x_below_zero"])
def test_fit_views_second_view_sees_one_row_in_one_wave(gpu, name, index):
    """Two views of the 257-point model.  The second frame is empty but for the pixel of one row, which sits at `index`: the first
    lane of each of the workgroup's four waves, and the first point of the second stride.  A kept row there sets the view's bit of
    views_used from that wave's ballot alone (0b11); a dropped row, whose relaxed compare would read an in-gate pixel, does not
    (0b01)."""
    ft, bank = gpu
    row = fe.BY_NAME[name]
    tb = table(257, 25.0, pin=(name, index))
    assert tb.index[name] == index
    frames = np.stack([tb.frames[0], fe.lone_frame(row)])
    Ks = np.stack([fe.K, fe.K])
    inst = view_instances(tb.inst, [0], [3])
    out, rec = run_views(ft, models_of(bank, 257, 25.0, False, tb, pin=(name, index)), frames, Ks, inst, 25.0, device=index == 128)
    got = (rec["points"][0], rec["sum_r2_fixed"][0], rec["views_used"][0])
    assert got == (tb.points + row.points, tb.e + row.e, 0b11 if row.points else 0b01), got
    same_records(rec, views_restated(frames, Ks, inst, tb.models, 25.0), "record")
    assert out.tobytes() == inst.tobytes()


# ---------------------------------------------------------------- the shape steps and the calibration step
def field_of(n):
    B = np.zeros((1, n, 3), np.float32)
    B[..., 2] = 1.0
    return B


def hold_sums(rec, points, e, what):
    assert (rec["points"], rec["sum_r2_fixed"], rec["reserved"]) == (points, e, 0), (what, rec, (points, e))


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("gate", fe.GATES)
def test_shape_steps_row_by_row(gpu, gate, mirrored):
    """shape_step through the camera table and shape_step_views through identity views: one call per row, each with the row's
    one-point model and the instance that names the row's frame (camera)."""
    ft, bank = gpu
    tb = table("rows", gate, mirrored)
    ms = bank.rows(tb, mirrored)
    prm, ref_prm = fit.shape_params(gate=gate), sr.params(gate=gate)
    B = field_of(1)
    frames4 = tb.frames[None]
    V, u = np.broadcast_to(EYE, (len(tb.Ks), 3, 3)), np.zeros((len(tb.Ks), 3), np.float32)
    vinst = view_instances(tb.inst, range(len(tb.inst)), [1] * len(tb.inst))
    with fit.ShapeBasis(B) as basis, identity_views(tb.Ks) as views:
        for i, r in enumerate(tb.rows):
            pts, nrm = tb.models[i]
            got = ft.shape_step(tb.frames, ms[i], basis, tb.inst[i:i + 1], views.cameras, params=prm)
            hold_sums(got[0], r.points, r.e, ("shape_step", r.name))
            assert got.tobytes() == sr.shape_step(tb.frames, tb.Ks, pts, nrm, B, tb.inst[i:i + 1], prm=ref_prm).tobytes(), r.name
            got = ft.shape_step_views(frames4, views, ms[i], basis, vinst[i:i + 1], params=prm)
            hold_sums(got[0], r.points, r.e, ("shape_step_views", r.name))
            assert got.tobytes() == svr.shape_step(frames4, tb.Ks, V, u, pts, nrm, B, vinst[i:i + 1], prm=ref_prm).tobytes(), r.name
            if r.K is None and r.t is None:
                got = ft.shape_step(tb.frames, ms[i], basis, tb.inst[i:i + 1], fe.K, params=prm)
                hold_sums(got[0], r.points, r.e, ("shape_step, one K", r.name))


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gate", fe.GATES)
def test_shape_steps_aggregated_host_and_device(gpu, gate, n, mirrored):
    ft, bank = gpu
    tb = table(n, gate, mirrored)
    model = models_of(bank, n, gate, mirrored, tb)[0]
    pts, nrm = tb.models[0]
    prm, ref_prm = fit.shape_params(gate=gate), sr.params(gate=gate)
    B = field_of(n)
    vinst = view_instances(tb.inst, [0], [1])
    want = sr.shape_step(tb.frames, fe.K, pts, nrm, B, tb.inst, prm=ref_prm)
    want_views = svr.shape_step(tb.frames[None], tb.Ks, EYE[None], np.zeros((1, 3), np.float32), pts, nrm, B, vinst, prm=ref_prm)
    hold_sums(want[0], tb.points, tb.e, "the restatement")
    assert want.tobytes() == want_views.tobytes()
    d_frames, whole = between_guards(tb.frames, GUARD, fe.BACK)
    with fit.ShapeBasis(B) as basis, identity_views(tb.Ks) as views:
        for what, got in (("shape_step", ft.shape_step(tb.frames, model, basis, tb.inst, fe.K, params=prm)),
                          ("shape_step, cameras", ft.shape_step(tb.frames, model, basis, tb.inst, views.cameras, params=prm)),
                          ("shape_step_device", host(ft.shape_step(d_frames, model, basis, to_device(tb.inst), fe.K, params=prm, device_out=True), SREC)),
                          ("shape_step_views", ft.shape_step_views(tb.frames[None], views, model, basis, vinst, params=prm)),
                          ("shape_step_views_device", host(ft.shape_step_views(d_frames[None], views, model, basis, to_device(vinst), params=prm,
                                                                                device_out=True), SREC))):
            hold_sums(got[0], tb.points, tb.e, what)
            assert got.tobytes() == want.tobytes(), what


def calib_prm(gate):
    return fit.calib_params(gate=gate, pivot=fe.T), cr.params(gate=gate, pivot=fe.T)


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("gate", fe.GATES)
def test_calibrate_step_row_by_row(gpu, gate, mirrored):
    """One call per row; the record of the row's camera carries its sums.  The pivot is the table's t, so pixel_65535, whose t is
    its own (65 m from the pivot, beyond DH_CALIB_MAX_ARM), is the one row that takes no part."""
    ft, bank = gpu
    tb = table("rows", gate, mirrored)
    ms = bank.rows(tb, mirrored)
    prm, ref_prm = calib_prm(gate)
    frames4 = tb.frames[None]
    V, u = np.broadcast_to(EYE, (len(tb.Ks), 3, 3)), np.zeros((len(tb.Ks), 3), np.float32)
    vinst = view_instances(tb.inst, range(len(tb.inst)), [1] * len(tb.inst))
    with identity_views(tb.Ks) as views:
        for i, r in enumerate(tb.rows):
            pts, nrm = tb.models[i]
            got = ft.calibrate_step(frames4, views, ms[i], vinst[i:i + 1], params=prm)
            part = r.t is None
            hold_sums(got[i], r.points if part else 0, r.e if part else 0, ("calibrate_step", r.name))
            assert got["points"].sum() == got["points"][i]
            assert got.tobytes() == cr.calib_step(frames4, tb.Ks, V, u, pts, nrm, vinst[i:i + 1], prm=ref_prm).tobytes(), r.name


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gate", fe.GATES)
def test_calibrate_step_aggregated_host_and_device(gpu, gate, n, mirrored):
    ft, bank = gpu
    tb = table(n, gate, mirrored)
    model = models_of(bank, n, gate, mirrored, tb)[0]
    prm, ref_prm = calib_prm(gate)
    vinst = view_instances(tb.inst, [0], [1])
    want = cr.calib_step(tb.frames[None], tb.Ks, EYE[None], np.zeros((1, 3), np.float32), *tb.models[0], vinst, prm=ref_prm)
    d_frames, whole = between_guards(tb.frames, GUARD, fe.BACK)
    with identity_views(tb.Ks) as views:
        got = ft.calibrate_step(tb.frames[None], views, model, vinst, params=prm)
        dev = host(ft.calibrate_step(d_frames[None], views, model, to_device(vinst), params=prm, device_out=True), CREC)
    for what, rec in (("host", got), ("device", dev)):
        hold_sums(rec[0], tb.points, tb.e, what)
        assert rec.tobytes() == want.tobytes(), what


# ---------------------------------------------------------------- the entry points that take a subject set
@contextlib.contextmanager
def subject_set(mesh, n, st):
    """The mesh form of the aggregated model as a set of one subject at zero coefficients: the base model, whose normals must be
    the table's.  st: the restated set, a surface set or not."""
    surface = hasattr(st, "offsets")
    with fit.ShapeBasis(field_of(n)) as basis, fit.Subjects(mesh.verts, mesh.tris, basis, 1, max_offset=16.0 if surface else None) as got:
        pts, nrm = got.read(0)
        assert pts.tobytes() == st.pts[0].tobytes() and nrm.tobytes() == st.nrm[0].tobytes()
        assert (pts == mesh.verts).all() and (nrm == mesh.table.models[0][1]).all()
        yield got


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gate", fe.GATES)
def test_shape_step_subjects_and_identify_subjects_aggregated(gpu, gate, n, mirrored):
    ft, _ = gpu
    mesh = fe.aggregated_mesh(n, gate, mirrored)
    tb = mesh.table
    st = sb.Set(mesh.verts, mesh.tris, field_of(n), 1)
    want = sb.shape_step(tb.frames, fe.K, st, tb.inst, prm=sr.params(gate=gate))
    w_sub, w_rec, _, w_scores = ir.identify(tb.frames, fe.K, st, fe.as_dicts(tb.inst), prm=ir.params(iterations=0, gate=gate))
    d_frames, whole = between_guards(tb.frames, GUARD, fe.BACK)
    with subject_set(mesh, n, st) as got:
        prm = fit.shape_params(gate=gate)
        for what, rec in (("host", ft.shape_step_subjects(tb.frames, got, tb.inst, fe.K, params=prm)),
                          ("device", host(ft.shape_step_subjects(d_frames, got, to_device(tb.inst), fe.K, params=prm, device_out=True), SREC))):
            hold_sums(rec[0], tb.points, tb.e, ("shape_step_subjects", what))
            assert rec.tobytes() == want.tobytes(), what
        iprm = fit.ident_params(iterations=0, gate=gate)
        sub, rec, poses, scores = ft.identify_subjects(tb.frames, got, tb.inst, fe.K, params=iprm, scores=True)
        d = ft.identify_subjects(d_frames, got, to_device(tb.inst), fe.K, params=iprm, scores=True, device_out=True)
        d_scores, d_rec, d_poses = host(d[3], REC).reshape(1, 1), host(d[1], _lib.IDENT_RECORD_DTYPE), host(d[2], INST)
    for what, sc, rc, ps in (("host", scores, rec, poses), ("device", d_scores, d_rec, d_poses)):
        got_score = (sc["points"][0, 0], sc["sum_r2_fixed"][0, 0], sc["steps"][0, 0], sc["status"][0, 0])
        assert got_score == (tb.points, tb.e, 0, fit.FIT_OK), (what, got_score)
        assert sc.tobytes() == w_scores.tobytes() and rc.tobytes() == w_rec.tobytes(), what
        assert ps.tobytes() == tb.inst.tobytes(), what
    assert sub.tobytes() == w_sub.tobytes()


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gate", fe.GATES)
def test_surface_step_subjects_aggregated(gpu, gate, n, mirrored):
    """min_cos2 = 0: the grazing test passes every point (c * c >= 0), the chain alone decides."""
    ft, _ = gpu
    mesh = fe.aggregated_mesh(n, gate, mirrored)
    tb = mesh.table
    st = ur.Set(mesh.verts, mesh.tris, field_of(n), 1)
    want = ur.surface_step(tb.frames, fe.K, st, fe.as_dicts(tb.inst), prm=ur.params(gate=gate, min_cos2=0.0))
    d_frames, whole = between_guards(tb.frames, GUARD, fe.BACK)
    prm = fit.surface_params(gate=gate, min_cos2=0.0)
    with subject_set(mesh, n, st) as got:
        for what, rec in (("host", ft.surface_step_subjects(tb.frames, got, tb.inst, fe.K, params=prm)),
                          ("device", host(ft.surface_step_subjects(d_frames, got, to_device(tb.inst), fe.K, params=prm, device_out=True), UREC))):
            assert (rec["points"][0], rec["sum_r2_fixed"][0], rec["instances"][0]) == (tb.points, tb.e, 1), (what, rec)
            assert rec.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_surface_step_subjects_grazing_rows(gpu, n, mirrored):
    """c * c == min_cos2 * |p|^2 exactly is kept, one step inside is kept, one step outside is dropped: 2 of the 3 rows at GRAZE
    and all 3 at min_cos2 = 0, through the kernel's staged and streamed paths, in the host form and the _device form between guard
    bands."""
    ft, _ = gpu
    mesh = fe.aggregated_mesh(n, 256.0, mirrored, only=fe.GRAZING)
    tb = mesh.table
    st = ur.Set(mesh.verts, mesh.tris, field_of(n), 1)
    d_frames, whole = between_guards(tb.frames, GUARD, fe.BACK)
    with subject_set(mesh, n, st) as got:
        for min_cos2, points in ((fe.GRAZE, 2), (0.0, 3)):
            want = ur.surface_step(tb.frames, fe.K, st, fe.as_dicts(tb.inst), prm=ur.params(gate=256.0, min_cos2=min_cos2))
            prm = fit.surface_params(gate=256.0, min_cos2=min_cos2)
            for what, rec in (("host", ft.surface_step_subjects(tb.frames, got, tb.inst, fe.K, params=prm)),
                              ("device", host(ft.surface_step_subjects(d_frames, got, to_device(tb.inst), fe.K, params=prm, device_out=True), UREC))):
                assert (rec["points"][0], rec["sum_r2_fixed"][0]) == (points, 0), (what, min_cos2, rec)
                assert rec.tobytes() == want.tobytes(), (what, min_cos2)
