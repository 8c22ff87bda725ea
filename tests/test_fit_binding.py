"""What a Fitter's nine methods hand to the library, without a GPU and without the library.  The fitter
gets fit_binding_calls' recording stand-in.  Every host form calls the export of the right name with as many arguments as
include/depthhead_hip.h declares, each of the kind its declared type asks for, and returns outputs of the dtypes, shapes and
initial fill of the contract.  Every _device form refuses frames that do not lie on the fitter's device before it calls anything,
and `fit.check_tensor`, which every tensor argument of a _device form goes through, refuses each argument in its own words for a
wrong count, a wrong element size, a view that is not contiguous and -- the right size, the wrong device -- a tensor that lies
elsewhere.  No GPU test passes such a tensor: here the refusal is the whole test, there it would depend on it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fit_binding_calls as fb
from depthhead_amd import _lib, fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "depthhead_hip.h")).read()
RINST, VINST, FREC, VFREC = _lib.RENDER_INSTANCE_DTYPE, _lib.VIEW_INSTANCE_DTYPE, _lib.FIT_RECORD_DTYPE, _lib.VIEW_FIT_RECORD_DTYPE
# kind -> (the export without its _cameras, the record dtypes of its outputs after the subjects of an identify call)
KINDS = {"fit": ("dh_fit_depth", (RINST, FREC)), "fit_views": ("dh_fit_depth_views", (VINST, VFREC)),
         "shape": ("dh_fit_shape", (_lib.SHAPE_RECORD_DTYPE,)), "shape_set": ("dh_fit_shape_subjects", (_lib.SHAPE_RECORD_DTYPE,)),
         "surface": ("dh_fit_surface_subjects", (_lib.SURFACE_RECORD_DTYPE,)), "shape_views": ("dh_fit_shape_views", (_lib.SHAPE_RECORD_DTYPE,)),
         "ident": ("dh_fit_identify_subjects", (_lib.IDENT_RECORD_DTYPE, RINST, FREC)),
         "ident_views": ("dh_fit_identify_subjects_views", (_lib.IDENT_RECORD_DTYPE, VINST, VFREC)),
         "calib": ("dh_fit_calibrate_views", (_lib.CALIB_RECORD_DTYPE,))}
FRAMES = "device frames: a contiguous 16-bit tensor on the fitter's device is expected"


def declared(name):
    """[(type, name)] of the export's parameters as the header declares them."""
    text = re.search(r"^int %s\((.*?)\);" % name, HEADER, re.S | re.M).group(1)
    return [re.match(r"(.*?)(\w+)(\[9\])?$", " ".join(p.split())).groups() for p in text.split(",")]


def test_every_host_form_calls_its_export_as_the_header_declares_it():
    rec = fb.Recorder()
    f = fb.fitter(fit, rec)
    seen = set()
    for label, call in fb.host_cases(fit, _lib):
        out = call(f)
        (name, args), = rec.calls
        rec.calls.clear()
        kind, cameras = label.split()[0], label.split()[1:2] == ["cameras"]
        export, dtypes = KINDS[kind]
        assert name == export + ("_cameras" if cameras else "") and name in _lib.EXPORTS, label
        seen.add(name)
        params = declared(name)
        assert len(args) == len(params), (label, len(args), params)
        value = {}
        for arg, (ctype, pname, array) in zip(args, params):
            if "*" in ctype or array:
                assert arg is None or isinstance(arg, (C.c_void_p, C.Array)) or type(arg).__name__ == "CArgObject", (label, pname, arg)
            elif ctype.strip() == "uint32_t":
                assert isinstance(arg, C.c_uint32), (label, pname, arg)
                value[pname] = arg.value
            else:
                assert ctype.strip() == "int" and type(arg) is int, (label, pname, arg)
        # the outputs: zeros of the record dtypes, IDENT_UNKNOWN for the subjects of an identify call, scores only where asked for
        out = out if isinstance(out, tuple) else (out,)
        ni, ns = value["n_instances"], value.get("n_subjects")
        shapes = {"shape": (ns,), "shape_set": (ns,), "surface": (ns,), "shape_views": (ns,), "calib": (3,)}.get(kind, (ni,))
        if kind.startswith("ident"):
            assert out[0].dtype == np.uint32 and out[0].shape == (ni,) and (out[0] == _lib.IDENT_UNKNOWN).all(), label
            assert len(out) in (3, 4) and (len(out) == 4) == ("scores" in label) == (args[-1] is not None), label
            if len(out) == 4:
                assert out[3].shape == (ni, ns), label
            out = out[1:]
        assert len(out) == len(dtypes) or kind.startswith("ident") and len(out) == 2, label
        for o, dtype in zip(out, dtypes):
            assert isinstance(o, np.ndarray) and o.dtype == dtype and not o.tobytes().strip(b"\0"), (label, o)
            assert o.shape == shapes or o.ndim == 2, (label, o.shape)
        if "no instances" in label:
            assert ni == 0 and args[[p[1] for p in params].index("instances")] is None, label
    assert seen == {export + c for export, _ in KINDS.values() for c in ("", "_cameras") if export + c in _lib.EXPORTS} and len(seen) == 14


def device_calls(f, frames, sets2):
    """Every kind's _device form with frames that are torch tensors."""
    h = fb.Handle
    cams, views, model, basis, subjects = h(2, 3), h(3, 3), h(4), h(5, 4), h(6, 3)
    inst, vinst = np.zeros(2, RINST), np.zeros(2, VINST)
    d_inst, d_vinst = torch.zeros(2 * RINST.itemsize, dtype=torch.uint8), torch.zeros(2 * VINST.itemsize, dtype=torch.uint8)
    K = np.eye(3)
    return [lambda: f.fit(frames, [model], inst, K, device_out=True),
            lambda: f.fit(frames, [model], inst, cams, device_out=True, carried=d_inst),
            lambda: f.fit_views(frames, [model], vinst, views, device_out=True),
            lambda: f.shape_step(frames, model, basis, d_inst, K, device_out=True),
            lambda: f.shape_step_subjects(frames, subjects, d_inst, cams, device_out=True),
            lambda: f.surface_step_subjects(frames, subjects, d_inst, K, device_out=True),
            lambda: f.identify_subjects(frames, subjects, d_inst, cams, scores=True, device_out=True),
            lambda: f.shape_step_views(sets2, views, model, basis, d_vinst, device_out=True),
            lambda: f.identify_subjects_views(sets2, views, subjects, d_vinst, device_out=True),
            lambda: f.calibrate_step(sets2, views, model, d_vinst, device_out=True)]


def test_every_device_form_refuses_frames_off_the_device_before_any_call():
    rec = fb.Recorder()
    f = fb.fitter(fit, rec)
    calls = device_calls(f, torch.zeros((3, fb.H, fb.W), dtype=torch.int16), torch.zeros((2, 3, fb.H, fb.W), dtype=torch.int16))
    for i, call in enumerate(calls):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == FRAMES, i
    assert rec.calls == []
    # the view count is refused before the frames, in each method's words
    four = torch.zeros((4, fb.H, fb.W), dtype=torch.int16)
    for i, call in enumerate(device_calls(f, four, four[None])):
        if i in (2, 7, 8, 9):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == ("4 frames for a view table of 3 cameras" if i == 2 else "4 frames a set for a view table of 3 cameras"), i
    assert rec.calls == []


WORDS = "device %s: a contiguous 32-bit tensor with one word per instance is expected"
# (name, dtype, per, the message, the torch dtype of a right tensor, one of another element size)
ARGUMENTS = [("subjects", np.uint32, "instance", WORDS % "subjects", torch.int32, torch.int64),
             ("sets", np.uint32, "instance", WORDS % "sets", torch.int32, torch.int16),
             ("take", np.uint32, "instance", WORDS % "take", torch.int32, torch.uint8),
             ("hold", np.uint8, "camera", "device hold: a contiguous 8-bit tensor with one byte per camera is expected", torch.uint8, torch.int16),
             ("enrolled", np.uint8, "subject", "device enrolled: a contiguous 8-bit tensor with one byte per subject is expected", torch.uint8, torch.int32),
             ("fit_records", FREC, "instance", "device fit_records: the contiguous tensor of one dh_fit_record per instance is expected", torch.uint8, None),
             ("fit_records", VFREC, "instance", "device fit_records: the contiguous tensor of one dh_view_fit_record per instance is expected",
              torch.uint8, None),
             ("carried", RINST, "instance", "carried: the contiguous device tensor of an earlier fit of as many instances is expected", torch.uint8, None)]


@pytest.mark.parametrize("name,dtype,per,message,right,other", ARGUMENTS, ids=[a[0] + "-" + str(np.dtype(a[1]).itemsize) for a in ARGUMENTS])
def test_check_tensor_refuses_each_argument_in_its_own_words(name, dtype, per, message, right, other):
    here, there, count = torch.device("cpu"), torch.device("cuda", 0), 5          # (making the device object needs no GPU)
    size = np.dtype(dtype).itemsize
    elements = count * size // torch.empty(0, dtype=right).element_size()

    def refused(t, device=here, n=count):
        with pytest.raises(ValueError) as e:
            fit.check_tensor(t, device, name, dtype, n, per)
        assert str(e.value) == message

    good = torch.zeros(elements, dtype=right)
    assert fit.check_tensor(good, here, name, dtype, count, per) is None
    refused(good, device=there)                                                    # the right size on the wrong device
    refused(good, n=count + 1)
    refused(good, n=count - 1)
    refused(torch.zeros(elements + 1, dtype=right))
    refused(torch.zeros(2 * elements, dtype=right)[::2])                           # the right count, not contiguous
    if other is not None:
        refused(torch.zeros(count, dtype=other))                                   # the right count of another element size
        refused(torch.zeros(count * size // torch.empty(0, dtype=other).element_size() or 1, dtype=other))   # (nearly) the right bytes
    else:
        assert fit.check_tensor(torch.zeros(count * size // 4, dtype=torch.int32), here, name, dtype, count, per) is None   # records: bytes alone


def test_check_tensor_on_frames_and_instances():
    here, there = torch.device("cpu"), torch.device("cuda", 0)
    frames = torch.zeros((2, 4, 6), dtype=torch.int16)
    assert fit.check_tensor(frames, here, "frames", np.uint16) is None
    for bad, device in ((frames, there), (frames[:, :, ::2], here), (frames.to(torch.int32), here), (frames.to(torch.uint8), here)):
        with pytest.raises(ValueError) as e:
            fit.check_tensor(bad, device, "frames", np.uint16)
        assert str(e.value) == FRAMES
    inst = torch.zeros(3 * RINST.itemsize, dtype=torch.uint8)
    assert fit.check_tensor(inst, here, "instances") is None
    for bad, device in ((inst, there), (inst[::2], here)):
        with pytest.raises(ValueError) as e:
            fit.check_tensor(bad, device, "instances")
        assert str(e.value) == "device instances: a contiguous tensor on the fitter's device is expected"


def test_the_shared_helpers():
    assert _lib.ref(None) is None and type(_lib.ref(_lib.FitParams())).__name__ == "CArgObject"
    assert _lib.stream_of(0, 77) == 77                                             # (no torch, no GPU: the default alone asks for them)
    kind, karg = _lib.intrinsics(fb.Handle(9))
    assert kind == "_cameras" and karg.value == 9
    kind, karg = _lib.intrinsics(np.arange(9.0).reshape(3, 3))
    assert kind == "" and isinstance(karg, C.c_void_p)
    assert (np.ctypeslib.as_array(C.cast(karg, C.POINTER(C.c_float)), (9,)) == np.arange(9, dtype=np.float32)).all()   # the array is still alive


def test_params_are_cast_by_the_fields_own_types(hip_lib):
    p = fit.fit_params(coarse_iterations=2.0, iterations=np.int64(3), gate=(50, np.float32(12.5)), lam=1, min_points=7.9)
    assert (p.coarse_iterations, p.iterations, tuple(p.gate), p.lam, p.min_points) == (2, 3, (50.0, 12.5), 1.0, 7)
    q = fit.fit_params()
    assert (p.reserved0, tuple(p.reserved)) == (q.reserved0, tuple(q.reserved)) and bytes(fit.fit_params(lam=q.lam)) == bytes(q)
    c = fit.calib_params(gate=30, pivot=np.array([1, 2, 3]), min_points=9)
    assert (c.gate, tuple(c.pivot), c.min_points, c.lam) == (30.0, (1.0, 2.0, 3.0), 9, fit.calib_params().lam)
    with pytest.raises(ValueError):
        fit.calib_params(pivot=(1.0, 2.0))
    t = fit.fit_track_params(iterations_tracked=3, rms_max=2, conf=(3, 7), max_coast=4.0)
    d = fit.fit_track_params()
    assert (t.iterations_tracked, t.rms_max, t.conf_num, t.conf_den, t.max_coast) == (3, 2.0, 3, 7, 4)
    assert (t.keep_points, t.max_jump, t.min_windows) == (d.keep_points, d.max_jump, d.min_windows)
    r = fit.rig_fit_track_params(max_misses=5, max_jump=40)
    assert (r.max_misses, r.max_jump, r.keep_points) == (5, 40.0, fit.rig_fit_track_params().keep_points)
    s = fit.surface_params(min_cos2=0.5, iterations=9)
    assert (s.min_cos2, s.iterations, s.gate) == (0.5, 9, fit.surface_params().gate)
    assert fit.shape_params(lam=2).lam == 2.0 and fit.ident_params(max_rms=np.inf).max_rms == np.inf
