"""A call's result does not depend on what its fitter ran before it: one sequence of host calls on one
shared Fitter visits all eight call kinds of the fit family -- fit, multi-view fit, shape step (plain and over a subject set),
surface step, identify, multi-view identify, multi-view shape step, calibration -- and every output of every call equals, byte
for byte, the same call on a fresh Fitter; one call of each kind also equals its _device form.  The sequence is ordered so that the
host staging grows in mid-sequence (one cropped frame first, two sets of three frames and the most instances later, the first
call again at the end), every nullable input is an array in one call and None in its neighbour of the same kind (an array that
changes the answer when it is read), and no size ends on a natural boundary (159 x 119 frames, 3 subjects, 5 and 7 instances).
The scene is ident_views_scenes' gallery of the 162-vertex head seen by three 160x120 cameras; its middle camera serves the
single-view kinds.  Before the last call the sequence runs the forms of the Python API that no other test drives (DESIGN.md section
18c): the shape step and the shape step over a set through a camera table, and a fit through one from carried poses, each against
its host form."""
import contextlib
import functools
import time

import numpy as np
import pytest

import ident_views_scenes as ivs
import shape_scenes as ss
import shape_views_scenes as svs
import surface_scenes as us
import view_fit_scenes as vs
from depthhead_amd import _lib, fit
from depthhead_amd.tracking import Cameras

pytestmark = pytest.mark.gpu

W, H, CW, CH, CAM = 160, 120, 159, 119, svs.MIDDLE
RINST, VINST, FREC, VFREC = _lib.RENDER_INSTANCE_DTYPE, _lib.VIEW_INSTANCE_DTYPE, _lib.FIT_RECORD_DTYPE, _lib.VIEW_FIT_RECORD_DTYPE
OUT = {"fit": (RINST, FREC), "fit_views": (VINST, VFREC), "shape": (_lib.SHAPE_RECORD_DTYPE,), "shape_set": (_lib.SHAPE_RECORD_DTYPE,),
       "surface": (_lib.SURFACE_RECORD_DTYPE,), "ident": (np.uint32, _lib.IDENT_RECORD_DTYPE, RINST, FREC),
       "ident_views": (np.uint32, _lib.IDENT_RECORD_DTYPE, VINST, VFREC), "shape_views": (_lib.SHAPE_RECORD_DTYPE,),
       "calib": (_lib.CALIB_RECORD_DTYPE,)}
IDENT = dict(min_points=16, max_rms=np.inf)


@functools.lru_cache(maxsize=None)
def scene():
    """(v, t, B, frames [2, 3, H, W], Ks, V, u, the restated set of 3, seven world instances -- of sets 0 1 0 1 1 0 1 --, the same
    seen through the middle camera alone: frame = set).  Set 0 shows subject 0, set 1 subject 2."""
    v, t, B, frames, Ks, V, u, inst, st = ivs.gallery("162", 3, W, H, [0, 2], sets=[0, 1, 0, 1, 1, 0, 1], masks=[0b111, 0b111, 0b011, 0b110, 0b101, 0b111, 0b011])
    world = svs.as_records(inst)
    single = ss.as_records([us.instance(i["set"], *vs.camera_pose(V[CAM], u[CAM], i["R"], i["t"])) for i in inst])
    return v, t, B, frames, Ks, V, u, st, world, np.array(ivs.sets_of(inst), np.uint32), single


@contextlib.contextmanager
def opened():
    """What the calls share on the GPU: the basis, the set in the restated one's state, the rig, and subject 1's model as the
    plain model of the fits, the shape steps and the calibration."""
    v, t, B, frames, Ks, V, u, st = scene()[:8]
    with contextlib.ExitStack() as stack:
        basis = stack.enter_context(fit.ShapeBasis(B))
        got = stack.enter_context(fit.Subjects(v, t, basis, 3))
        got.set_coeffs(st.state["coeffs"][:, :len(B)])
        cams = stack.enter_context(Cameras(Ks))
        yield dict(basis=basis, set=got, views=stack.enter_context(fit.Views(cams, V, u)), model=stack.enter_context(fit.Model(st.pts[1], st.nrm[1])),
                   coeffs=st.state["coeffs"][:, :len(B)], twice=stack.enter_context(Cameras(np.stack([Ks[CAM], Ks[CAM]]))))


@pytest.fixture(scope="module")
def world():
    with opened() as g:
        yield g


def d16(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).copy()).cuda()


def d8(array):
    import torch
    return None if array is None else torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).cuda()


def d32(words):
    import torch
    return None if words is None else torch.from_numpy(np.asarray(words, np.uint32).view(np.int32).copy()).cuda()


def run(f, g, kind, a, device=False):
    """One call of `kind` with the arguments `a` on fitter f, in the host form or the _device form: the tuple of its outputs.  The
    single-view kinds see through the middle camera's K or, with a["cameras"], through a table that holds it once per frame; with
    a["carried"] the _device fit gets the instances as an earlier fit's tensor and, as its instances, the same 50 mm away: it equals
    the host form only if it starts from the carried poses."""
    fr_ = d16(a["frames"]) if device else np.ascontiguousarray(a["frames"])
    words = d32 if device else (lambda x: x)
    rows = d8 if device else (lambda x: x)
    K = g["twice"] if a.get("cameras") else scene()[4][CAM]
    kw = dict(device_out=True) if device else {}
    if kind == "fit" and device and a.get("carried"):
        away = a["inst"].copy()
        away["t"] += np.float32(50.0)
        out = f.fit(fr_, [g["model"]], away, K, carried=d8(a["inst"]), **kw)
    elif kind == "fit":
        out = f.fit(fr_, [g["model"]], a["inst"], K, **kw)
    elif kind == "fit_views":
        out = f.fit_views(fr_, [g["model"]], a["inst"], g["views"], **kw)
    elif kind == "shape":
        out = f.shape_step(fr_, g["model"], g["basis"], rows(a["inst"]), K, subjects=words(a.get("subjects")), n_subjects=a["n_subjects"], **kw)
    elif kind == "shape_set":
        out = f.shape_step_subjects(fr_, g["set"], rows(a["inst"]), K, subjects=words(a.get("subjects")), n_subjects=a["n_subjects"],
                                    fit_records=rows(a.get("fit_records")), **kw)
    elif kind == "surface":                                    # (the step moves its set: each call takes a set of its own)
        with fit.Subjects(*scene()[:2], g["basis"], 3, max_offset=16.0) as surface:
            surface.set_coeffs(g["coeffs"])
            out = f.surface_step_subjects(fr_, surface, rows(a["inst"]), K, subjects=words(a.get("subjects")), n_subjects=a["n_subjects"],
                                          fit_records=rows(a.get("fit_records")), params=fit.surface_params(min_points=16), **kw)
            if device:
                out = out.cpu()
    elif kind == "ident":
        out = f.identify_subjects(fr_, g["set"], rows(a["inst"]), K, n_subjects=3, enrolled=rows(a.get("enrolled")), fit_records=rows(a.get("fit_records")),
                                  params=fit.ident_params(**IDENT), scores=True, **kw)
    elif kind == "ident_views":
        out = f.identify_subjects_views(fr_, g["views"], g["set"], rows(a["inst"]), sets=words(a.get("sets")), n_subjects=3, enrolled=rows(a.get("enrolled")),
                                        fit_records=rows(a.get("fit_records")), params=fit.ident_views_params(**IDENT), scores=True, **kw)
    elif kind == "shape_views":
        out = f.shape_step_views(fr_, g["views"], g["model"], g["basis"], rows(a["inst"]), sets=words(a.get("sets")), subjects=words(a.get("subjects")),
                                 n_subjects=a["n_subjects"], **kw)
    else:
        out = f.calibrate_step(fr_, g["views"], g["model"], rows(a["inst"]), sets=words(a.get("sets")), take=words(a.get("take")), hold=rows(a.get("hold")), **kw)
    out = out if isinstance(out, tuple) else (out,)
    if device:
        import torch
        torch.cuda.synchronize()
        out = tuple(o.cpu().numpy().view(np.uint8).view(dt) for o, dt in zip(out, OUT[kind]))
    return tuple(np.ascontiguousarray(o).reshape(-1) for o in out)


def staged(a, out):
    """The bytes a host call stages on the device: every array it passes and every array it returns, each rounded up to 256."""
    return sum(-(-np.asarray(x).nbytes // 256) * 256 for x in list(a.values()) + list(out) if isinstance(x, np.ndarray))


def sequence():
    """[(kind, arguments, whether the _device form is compared too)], in the order of the docstring above."""
    frames, world, sets, single = scene()[3], scene()[8], scene()[9], scene()[10]
    one, two = np.ascontiguousarray(frames[:1, CAM, :CH, :CW]), np.ascontiguousarray(frames[:, CAM, :CH, :CW])
    rig1, rig2 = frames[0], np.ascontiguousarray(frames[:, :, :CH, :CW])
    first = single[sets == 0][:1]
    bad = np.zeros(5, FREC)
    bad["status"][[1, 3]] = fit.FIT_FEW_POINTS
    vbad = np.zeros(7, VFREC)
    vbad["status"][[0, 4]] = fit.FIT_FEW_POINTS
    subj = np.array([0, 2, 1, 2, _lib.SHAPE_SKIP], np.uint32)
    take = np.array([0, _lib.CALIB_SKIP, 0, 0, _lib.CALIB_SKIP], np.uint32)
    return [
        ("fit", dict(frames=one, inst=first), True),
        ("ident", dict(frames=two, inst=single[:5]), False),
        ("ident", dict(frames=two, inst=single[:5], enrolled=np.array([0, 1, 1], np.uint8), fit_records=bad), True),   # subject 0 masked
        ("shape", dict(frames=two, inst=single[:5], n_subjects=1), False),
        ("shape", dict(frames=two, inst=single[:5], subjects=subj, n_subjects=3), True),
        ("shape_set", dict(frames=two, inst=single[:5], subjects=subj, n_subjects=3), False),
        ("shape_set", dict(frames=two, inst=single[:5], n_subjects=3, fit_records=bad), True),
        ("surface", dict(frames=two, inst=single[:5], subjects=subj, n_subjects=3, fit_records=bad), True),
        ("surface", dict(frames=two, inst=single[:5], n_subjects=3), False),
        ("fit_views", dict(frames=rig1, inst=world[sets == 0]), True),
        ("ident_views", dict(frames=frames, inst=world, sets=sets), False),                                              # the largest call
        ("ident_views", dict(frames=frames, inst=world, enrolled=np.array([0, 1, 1], np.uint8), fit_records=vbad), True),   # all in set 0
        ("shape_views", dict(frames=rig2, inst=world[:5], sets=sets[:5], subjects=subj, n_subjects=3), True),
        ("shape_views", dict(frames=rig2, inst=world[:5], n_subjects=1), False),
        ("calib", dict(frames=rig2, inst=world[:5], sets=sets[:5], take=take, hold=np.array([0, 1, 0], np.uint8)), True),
        ("calib", dict(frames=rig2, inst=world[:5]), False),
        # the forms of the Python API that no other test runs: the _cameras twins of the shape steps, and of a carried fit, on the device
        ("shape", dict(frames=two, inst=single[:5], subjects=subj, n_subjects=3, cameras=True), True),
        ("shape_set", dict(frames=two, inst=single[:5], subjects=subj, n_subjects=3, fit_records=bad, cameras=True), True),
        ("fit", dict(frames=two, inst=single[:5], cameras=True, carried=True), True),
        ("fit", dict(frames=one, inst=first), False),
    ]


def test_every_call_kind_interleaved_on_one_fitter_against_a_fresh_fitter_and_the_device_form(world):
    calls = sequence()
    with fit.Fitter() as shared:
        for _ in range(2):                                     # (the second pass is the timed one: its staging no longer grows)
            t0 = time.perf_counter()
            got = [run(shared, world, kind, a) for kind, a, _ in calls]
            print("the sequence of %d host calls: %.1f ms" % (len(calls), 1e3 * (time.perf_counter() - t0)))
            for i, (kind, a, device) in enumerate(calls):
                with fit.Fitter() as fresh:
                    want = run(fresh, world, kind, a)
                    assert len(got[i]) == len(want) == len(OUT[kind])
                    for o, w_ in zip(got[i], want):
                        assert o.dtype == w_.dtype and o.tobytes() == w_.tobytes(), (i, kind, o, w_)
                    if device:
                        for o, w_ in zip(run(fresh, world, kind, a, device=True), want):
                            assert o.tobytes() == w_.tobytes(), (i, kind, "the _device form", o, w_)
    # ---- the sequence is what the docstring says it is
    need = [staged(a, o) for (_, a, _), o in zip(calls, got)]
    big = [kind for kind, _, _ in calls].index("ident_views")
    kept = max(need[:big])
    assert need[big] >= max(need) - 256 and 0 < big < len(calls) - 1
    assert need[big] > kept + kept // 4 + 4096, (need, "the largest call must outgrow the headroom of every call before it")
    assert need[0] == need[-1] == min(need) and calls[0][1]["frames"].size % 2 == 1
    assert len(calls[big][1]["inst"]) > max(len(a["inst"]) for _, a, _ in calls[:big])
    # every array that alternates with None changes the answer, so reading a stale one in its place would show
    for i, j in ((1, 2), (3, 4), (5, 6), (7, 8), (10, 11), (12, 13), (14, 15)):
        assert calls[i][0] == calls[j][0] and b"".join(o.tobytes() for o in got[i]) != b"".join(o.tobytes() for o in got[j]), (i, j)
    assert got[1][0][0] == 0 and got[2][0][0] != 0                             # the mask hides the true subject of instance 0
    assert got[10][0].tolist() != got[11][0].tolist()
