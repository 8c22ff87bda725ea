"""The calibration entry points without a GPU: exported and declared, the two structs laid out as the
header states, the defaults, and every refusal that is decided before a device is touched answers DH_EINVAL with a message that
names the call and leaves the records untouched.  Models and view tables live on a device, so where a refusal only needs a
handle that is not NULL the calls get a block that reads as one: zeros for a model (0 points on device 0), and for the view
table two words and a pointer (device, n cameras, its camera table: again two words, device and n) -- every refusal tested here
is decided before the handle's device memory would be used.  The refusals that need a real model (the extent, the term limits)
are in tests/test_gpu_calibrate.py."""
import ctypes as C
import re

import numpy as np

import abi_kit
from abi_kit import err as _err, Cameras as FakeCameras, Model as FakeModel, Views as FakeViews
from depthhead_amd import _lib

NEW = ["dh_calib_params_default", "dh_fit_calibrate_views", "dh_fit_calibrate_views_device"]
EINVAL = -1


def test_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    from depthhead_amd import fit
    assert callable(fit.Fitter.calibrate_step) and callable(fit.calibrate_views) and callable(fit.views_from_records)
    assert callable(fit.calib_params)
    assert (fit.CALIB_OK, fit.CALIB_FEW_POINTS, fit.CALIB_SINGULAR, fit.CALIB_NOT_ORTHONORMAL, fit.CALIB_HELD) == (0, 1, 2, 3, 4)


def test_header_and_exports_are_equal():
    text = abi_kit.header()
    abi_kit.assert_header_equals_exports(NEW, "calibrating a view table")
    # the two declarations differ in the stream alone
    host = re.search(r"int dh_fit_calibrate_views\((.*?)\);", text, re.S).group(1)
    device = re.search(r"int dh_fit_calibrate_views_device\((.*?)\);", text, re.S).group(1)
    assert " ".join(device.split()) == " ".join(host.split()) + ", void *stream"
    for name, value in (("DH_CALIB_OK", "0u"), ("DH_CALIB_FEW_POINTS", "1u"), ("DH_CALIB_SINGULAR", "2u"), ("DH_CALIB_NOT_ORTHONORMAL", "3u"),
                        ("DH_CALIB_HELD", "4u"), ("DH_CALIB_SKIP", "0xFFFFFFFFu"), ("DH_CALIB_ARM_UNIT", "64.0"), ("DH_CALIB_MAX_ARM", "2048.0")):
        assert re.search(rf"#define {name} {re.escape(value)}\s", text), name
    assert (_lib.CALIB_SKIP, _lib.CALIB_ARM_UNIT, _lib.CALIB_MAX_ARM) == (0xFFFFFFFF, 64, 2048)


def test_struct_layouts():
    d = _lib.CALIB_RECORD_DTYPE
    assert d.itemsize == 120
    assert [(n, d.fields[n][1]) for n in d.names] == [("V", 0), ("u", 36), ("points", 48), ("pairs", 52), ("status", 56), ("reserved", 60),
                                                      ("sum_r2_fixed", 64), ("delta", 72)]
    assert d["V"].shape == (9,) and d["u"].shape == (3,) and d["delta"].shape == (6,)
    assert sum(d[n].itemsize for n in d.names) == 120                    # no padding
    P = _lib.CalibParams
    assert C.sizeof(P) == 64
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("gate", 0), ("lam", 8), ("pivot", 16), ("min_points", 40), ("reserved0", 44),
                                                                  ("reserved", 48)]
    # the struct of the header, field for field
    text = abi_kit.header()
    body = re.search(r"typedef struct dh_calib_record \{(.*?)\} dh_calib_record;", text, re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+([^;]+);", body, re.M)
    assert [(t, " ".join(n.split())) for t, n in fields] == [("float", "V[9], u[3]"), ("uint32_t", "points"), ("uint32_t", "pairs"), ("uint32_t", "status"),
                                                             ("uint32_t", "reserved"), ("int64_t", "sum_r2_fixed"), ("double", "delta[6]")]
    body = re.search(r"typedef struct dh_calib_params \{(.*?)\} dh_calib_params;", text, re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+([^;]+);", body, re.M)
    assert [(t, n) for t, n in fields] == [("double", "gate"), ("double", "lambda"), ("double", "pivot[3]"), ("uint32_t", "min_points"),
                                           ("uint32_t", "reserved0"), ("uint64_t", "reserved[2]")]


def test_defaults(hip_lib):
    p = _lib.CalibParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert hip_lib.dh_calib_params_default(C.byref(p)) == 0
    assert (p.gate, p.lam, p.min_points, list(p.pivot), p.reserved0, list(p.reserved)) == (25.0, 1e-3, 64, [0.0, 0.0, 0.0], 0, [0, 0])
    assert hip_lib.dh_calib_params_default(None) == EINVAL and "dh_calib_params_default" in hip_lib.dh_last_error().decode()
    from depthhead_amd import fit
    q = fit.calib_params(gate=60.0, lam=0.0, min_points=7, pivot=(1.0, -2.0, 3.5))
    assert (q.gate, q.lam, q.min_points, list(q.pivot)) == (60.0, 0.0, 7, [1.0, -2.0, 3.5])


def test_refusals_leave_the_records_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    frames = np.full((2, 3, 8, 8), 800, np.uint16)
    rec = np.full(3 * 120, 0xCD, np.uint8)
    zeros = np.zeros(256, np.uint8)
    cams = FakeCameras(0, 3)
    table = FakeViews(0, 3, C.addressof(cams))
    views = C.addressof(table)
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value

    def inst(first_cam=0, mask=0b111):
        a = np.zeros(1, _lib.VIEW_INSTANCE_DTYPE)
        a["first_cam"], a["views"], a["scale"] = first_cam, mask, 1.0
        a["R"][0] = np.eye(3, dtype=np.float32).reshape(9)
        a["t"][0] = (0, 0, 800)
        return a

    def calls(f, ins, n_sets, w, h, prm, fr=frames, r=rec, vw=views, mdl=zeros, sets=None, take=None, hold=None, device_too=True, ni=None):
        p = C.byref(prm) if prm is not None else None
        ni = (0 if ins is None else len(ins)) if ni is None else ni
        yield "dh_fit_calibrate_views", lib.dh_fit_calibrate_views(f, vp(fr), n_sets, w, h, vp(vw), vp(mdl), vp(ins), ni, vp(sets), vp(take), vp(hold), p,
                                                                   vp(r))
        if device_too:
            yield "dh_fit_calibrate_views_device", lib.dh_fit_calibrate_views_device(f, vp(fr), n_sets, w, h, vp(vw), vp(mdl), vp(ins), ni, vp(sets), vp(take),
                                                                                     vp(hold), p, vp(r), None)

    def refused(what, *args, **kw):
        for name, rc in calls(*args, **kw):
            assert rc == EINVAL and what in _err(lib) and name + ":" in _err(lib), (name, rc, _err(lib))
        assert (rec == 0xCD).all()

    def with_params(**kw):
        p = _lib.CalibParams()
        assert lib.dh_calib_params_default(C.byref(p)) == 0
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            elif k == "pivot":
                p.pivot[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    prm = with_params()
    refused("NULL fitter", None, None, 2, 8, 8, prm)
    refused("NULL frames", ft, None, 2, 8, 8, prm, fr=None)
    refused("NULL records", ft, None, 2, 8, 8, prm, r=None)
    refused("NULL model", ft, None, 2, 8, 8, prm, mdl=None)
    refused("NULL view table", ft, None, 2, 8, 8, prm, vw=None)
    elsewhere = FakeViews(1, 3, C.addressof(cams))
    refused("the view table lives on device 1", ft, None, 2, 8, 8, prm, vw=C.addressof(elsewhere))
    far_model = FakeModel(1, 0, 0.0)
    refused("the model lives on device 1", ft, None, 2, 8, 8, prm, mdl=C.addressof(far_model))
    refused("n_sets = 0", ft, None, 0, 8, 8, prm)
    refused("n_sets = 21846", ft, None, 21846, 8, 8, prm)                 # 21846 * 3 = 65538; 21845 * 3 = 65535 passes this test
    refused("frame size", ft, None, 21845, 0, 8, prm)
    refused("n_sets = 4294967295", ft, None, 0xFFFFFFFF, 8, 8, prm)
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, _lib.RENDER_MAX_SIZE + 1), (_lib.RENDER_MAX_SIZE + 1, 8)):
        refused("frame size", ft, None, 2, w, h, prm)
    for v in (0.0, -1.0, 256.5, np.nan, np.inf):
        refused("gate", ft, None, 2, 8, 8, with_params(gate=v))
    for v in (-1e-9, np.nan, np.inf):
        refused("lambda", ft, None, 2, 8, 8, with_params(lam=v))
    refused("min_points 0", ft, None, 2, 8, 8, with_params(min_points=0))
    for axis in range(3):
        for v in (np.nan, np.inf, -np.inf):
            refused(f"pivot[{axis}]", ft, None, 2, 8, 8, with_params(pivot=(axis, v)))
    for kw in (dict(reserved0=1), dict(reserved=0), dict(reserved=1)):
        refused("reserved", ft, None, 2, 8, 8, with_params(**kw))
    refused("NULL instances", ft, None, 2, 8, 8, None, ni=1)
    refused("too many instances", ft, inst(), 2, 8, 8, None, ni=(1 << 23) + 1)
    # the host form's per-instance refusals (the _device form cannot read the instances: the device skips these)
    host = dict(device_too=False)
    refused("instance 0 is seen by no view", ft, inst(mask=0), 2, 8, 8, prm, **host)
    refused("names camera 3 of 3", ft, inst(mask=0b1000), 2, 8, 8, prm, **host)
    refused("names camera 3 of 3", ft, inst(first_cam=2, mask=0b11), 2, 8, 8, prm, **host)
    refused("names camera 63 of 3", ft, inst(mask=(1 << 63) | 1), 2, 8, 8, prm, **host)
    refused("names camera 4294967296 of 3", ft, inst(first_cam=0xFFFFFFFF, mask=0b10), 2, 8, 8, prm, **host)
    refused("names set 2 of 2", ft, inst(), 2, 8, 8, prm, sets=np.array([2], np.uint32), **host)
    refused("names set 4294967295 of 2", ft, inst(), 2, 8, 8, prm, sets=np.array([0xFFFFFFFF], np.uint32), **host)
    # the order: the view, the camera, the set, then R, t and scale; any take but DH_CALIB_SKIP takes part
    bad = inst(mask=0)
    bad["R"][0, 0] = np.nan
    nine = np.array([9], np.uint32)
    refused("seen by no view", ft, bad, 2, 8, 8, prm, sets=nine, take=nine, **host)
    bad["views"] = 0b1000
    refused("names camera 3", ft, bad, 2, 8, 8, prm, sets=nine, take=nine, **host)
    bad["views"] = 0b1
    refused("names set 9", ft, bad, 2, 8, 8, prm, sets=nine, take=nine, **host)
    refused("non-finite R, t or scale", ft, bad, 2, 8, 8, prm, take=nine, **host)
    refused("non-finite R, t or scale", ft, bad, 2, 8, 8, prm, take=np.array([0xFFFFFFFE], np.uint32), **host)
    for field, idx in (("R", 4), ("t", 2), ("scale", None)):
        for x in (np.nan, np.inf, -np.inf):
            a = inst()
            if idx is None:
                a[field][0] = x
            else:
                a[field][0, idx] = x
            refused("non-finite R, t or scale", ft, a, 2, 8, 8, prm, **host)
    for idx, x, where in ((7, -2.5, "[1][2]"), (0, 1.011, "[0][0]"), (1, 0.021, "[0][1]")):
        a = inst()
        a["R"][0, idx] = x
        refused(f"not orthonormal: (R R^T){where}", ft, a, 2, 8, 8, prm, **host)
    # a refusal holds for a held camera's instance too: holding a camera leaves pairs out, not instances
    refused("names set 2 of 2", ft, inst(), 2, 8, 8, prm, sets=np.array([2], np.uint32), hold=np.ones(3, np.uint8), **host)
    assert (rec == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0
