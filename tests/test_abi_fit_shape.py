"""The shape entry points without a GPU: exported and declared, the dh_shape_params / dh_shape_record layouts
of the Python side equal the C layout (a g++ program prints sizeof and offsetof from include/depthhead_hip.h), the defaults, and
every refusal that is decided before a device is touched answers DH_EINVAL with a message and leaves the records untouched.
Models and bases live on a device, so where a refusal only needs a handle that is not NULL the calls get a block of zeros:
every refusal tested here is decided before the handle's device memory would be used (a model of 0 points on device 0).  The
refusals that need a real model or basis (another n, the field limit, the term limit) are in tests/test_gpu_fit_shape.py."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_fit_basis_create", "dh_fit_basis_destroy", "dh_fit_basis_info", "dh_shape_params_default", "dh_fit_shape", "dh_fit_shape_cameras",
       "dh_fit_shape_device", "dh_fit_shape_cameras_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_shape_params size %zu\n", sizeof(dh_shape_params));
    F(dh_shape_params, gate); F(dh_shape_params, lambda); F(dh_shape_params, min_points); F(dh_shape_params, reserved0); F(dh_shape_params, reserved);
    printf("dh_shape_record size %zu\n", sizeof(dh_shape_record));
    F(dh_shape_record, delta); F(dh_shape_record, points); F(dh_shape_record, instances); F(dh_shape_record, status); F(dh_shape_record, reserved);
    F(dh_shape_record, sum_r2_fixed);
    printf("consts %u %u %u %u %u %u %d %d %u\n", DH_SHAPE_OK, DH_SHAPE_FEW_POINTS, DH_SHAPE_SINGULAR, DH_SHAPE_MAX_FIELDS, DH_SHAPE_MAX_SUBJECTS,
           DH_SHAPE_SKIP, (int)DH_SHAPE_MAX_FIELD, (int)DH_SHAPE_MAX_GATE, DH_SHAPE_MAX_TERMS);
    return 0;
}
"""


def test_shape_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    import depthhead_amd
    from depthhead_amd import fit, synth
    assert hasattr(depthhead_amd, "ShapeBasis") and "ShapeBasis" in depthhead_amd.__all__
    for name in ("ShapeBasis", "shape_params", "deform", "adapt"):
        assert callable(getattr(fit, name)), name
    assert callable(fit.Fitter.shape_step) and callable(synth.head_basis)
    assert fit.SHAPE_RECORD_DTYPE is _lib.SHAPE_RECORD_DTYPE
    assert (fit.SHAPE_OK, fit.SHAPE_FEW_POINTS, fit.SHAPE_SINGULAR) == (0, 1, 2)


def test_header_and_exports_are_equal():
    abi_kit.assert_header_equals_exports(NEW)


def test_layouts_match_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [int(v) for v in consts]
    assert consts == [0, 1, 2, _lib.SHAPE_MAX_FIELDS, _lib.SHAPE_MAX_SUBJECTS, _lib.SHAPE_SKIP, _lib.SHAPE_MAX_FIELD, _lib.SHAPE_MAX_GATE,
                      _lib.SHAPE_MAX_TERMS] == [0, 1, 2, 8, 256, 0xFFFFFFFF, 256, 256, 1 << 23]
    dt = _lib.SHAPE_RECORD_DTYPE
    assert c[("dh_shape_record", "size")] == dt.itemsize == 88 == sum(dt.fields[f][0].itemsize for f in dt.names)      # no padding
    for f in dt.names:
        assert c[("dh_shape_record", f)] == dt.fields[f][1], f
    assert c[("dh_shape_params", "size")] == C.sizeof(_lib.ShapeParams) == 40
    for f, _ in _lib.ShapeParams._fields_:
        assert c[("dh_shape_params", "lambda" if f == "lam" else f)] == getattr(_lib.ShapeParams, f).offset, f


def default_params(lib):
    p = _lib.ShapeParams()
    assert lib.dh_shape_params_default(C.byref(p)) == 0
    return p


def test_default_params(hip_lib):
    p = default_params(hip_lib)
    assert (p.gate, p.lam, p.min_points, p.reserved0, list(p.reserved)) == (25.0, 1e-3, 64, 0, [0, 0])
    assert hip_lib.dh_shape_params_default(None) == EINVAL and "NULL" in _err(hip_lib)


def test_basis_create_refusals(hip_lib):
    lib, vp = hip_lib, _lib.vp
    B = np.ones((2, 3, 3), np.float32)
    h = C.c_void_p(1234)
    assert lib.dh_fit_basis_create(None, 3, 2, 0, C.byref(h)) == EINVAL and "NULL" in _err(lib) and h.value is None
    assert lib.dh_fit_basis_create(vp(B), 3, 2, 0, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_fit_basis_create(vp(B), 0, 2, 0, C.byref(h)) == EINVAL and "0 points" in _err(lib)
    assert lib.dh_fit_basis_create(vp(B), _lib.FIT_MAX_POINTS + 1, 2, 0, C.byref(h)) == EINVAL and "32769 points" in _err(lib)
    assert lib.dh_fit_basis_create(vp(B), 3, 0, 0, C.byref(h)) == EINVAL and "0 fields" in _err(lib)
    assert lib.dh_fit_basis_create(vp(B), 3, 9, 0, C.byref(h)) == EINVAL and "9 fields" in _err(lib)
    assert lib.dh_fit_basis_create(vp(B), 3, 2, -1, C.byref(h)) == EINVAL and "device -1" in _err(lib)
    for x in (np.nan, np.inf, -np.inf):
        w = B.copy(); w[1, 2, 0] = x
        assert lib.dh_fit_basis_create(vp(w), 3, 2, 0, C.byref(h)) == EINVAL and "field 1 has a value at point 2" in _err(lib)
    assert h.value is None
    assert lib.dh_fit_basis_destroy(None) == 0
    assert lib.dh_fit_basis_info(None, None, None, None) == EINVAL and "NULL" in _err(lib)


def test_shape_refusals_leave_the_records_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    K = np.array([100, 0, 4, 0, 100, 4, 0, 0, 1], np.float32)
    frames = np.full((2, 8, 8), 800, np.uint16)
    rec = np.full(2 * 88, 0xCD, np.uint8)
    zeros = np.zeros(256, np.uint8)                      # a handle that is not NULL: a model / basis of 0 points on device 0
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value

    def inst(frame=0):
        a = np.zeros(1, _lib.RENDER_INSTANCE_DTYPE)
        a["frame"], a["scale"] = frame, 1.0
        a["R"][0] = np.eye(3, dtype=np.float32).reshape(9)
        a["t"][0] = (0, 0, 800)
        return a

    def calls(f, ins, n, w, h, prm, fr=frames, r=rec, k=K, mdl=zeros, bas=zeros, subj=None, ns=1, device_too=True):
        p = C.byref(prm) if prm is not None else None
        ni = 0 if ins is None else len(ins)
        yield "dh_fit_shape", lib.dh_fit_shape(f, vp(fr), n, w, h, vp(k), vp(mdl), vp(bas), vp(ins), ni, vp(subj), ns, p, vp(r))
        if device_too:
            yield "dh_fit_shape_device", lib.dh_fit_shape_device(f, vp(fr), n, w, h, vp(k), vp(mdl), vp(bas), vp(ins), ni, vp(subj), ns, p, vp(r), None)

    def refused(what, *args, **kw):
        for name, rc in calls(*args, **kw):
            assert rc == EINVAL and what in _err(lib) and name in _err(lib), (name, rc, _err(lib))
        assert (rec == 0xCD).all()

    prm = default_params(lib)
    refused("NULL fitter", None, None, 2, 8, 8, prm)
    refused("NULL frames", ft, None, 2, 8, 8, prm, fr=None)
    refused("NULL records", ft, None, 2, 8, 8, prm, r=None)
    refused("NULL model", ft, None, 2, 8, 8, prm, mdl=None)
    refused("NULL basis", ft, None, 2, 8, 8, prm, bas=None)
    refused("NULL K", ft, None, 2, 8, 8, prm, k=None)
    for n in (0, -1, 65536):
        refused("frames", ft, None, n, 8, 8, prm)
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, _lib.RENDER_MAX_SIZE + 1), (_lib.RENDER_MAX_SIZE + 1, 8)):
        refused("frame size", ft, None, 2, w, h, prm)
    for ns in (0, 257, 0xFFFFFFFF):
        refused("n_subjects", ft, None, 2, 8, 8, prm, ns=ns)

    def with_params(**kw):
        p = default_params(lib)
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    for v in (0.0, -1.0, 256.5, np.nan, np.inf):
        refused("gate", ft, None, 2, 8, 8, with_params(gate=v))
    for v in (-1e-9, np.nan, np.inf):
        refused("lambda", ft, None, 2, 8, 8, with_params(lam=v))
    refused("min_points 0", ft, None, 2, 8, 8, with_params(min_points=0))
    refused("reserved", ft, None, 2, 8, 8, with_params(reserved0=1))
    refused("reserved", ft, None, 2, 8, 8, with_params(reserved=0))
    refused("reserved", ft, None, 2, 8, 8, with_params(reserved=1))
    assert lib.dh_fit_shape(ft, vp(frames), 2, 8, 8, vp(K), vp(zeros), vp(zeros), None, 1, None, 1, None, vp(rec)) == EINVAL
    assert "NULL instances" in _err(lib)
    assert lib.dh_fit_shape_device(ft, vp(frames), 2, 8, 8, vp(K), vp(zeros), vp(zeros), None, 1, None, 1, None, vp(rec), None) == EINVAL
    assert "NULL instances" in _err(lib)
    assert lib.dh_fit_shape(ft, vp(frames), 2, 8, 8, vp(K), vp(zeros), vp(zeros), vp(inst()), (1 << 23) + 1, None, 1, None, vp(rec)) == EINVAL
    assert "too many instances" in _err(lib)
    # the host forms' per-instance refusals (the _device forms cannot read the instances: the device skips these)
    host = dict(device_too=False)
    refused("names frame 2 of 2", ft, inst(frame=2), 2, 8, 8, prm, **host)
    refused("names frame 4294967295 of 2", ft, inst(frame=0xFFFFFFFF), 2, 8, 8, prm, **host)
    refused("names subject 1 of 1", ft, inst(), 2, 8, 8, prm, subj=np.array([1], np.uint32), **host)
    refused("names subject 4294967294 of 1", ft, inst(), 2, 8, 8, prm, subj=np.array([0xFFFFFFFE], np.uint32), **host)
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
    for name, fn in (("dh_fit_shape_cameras", lib.dh_fit_shape_cameras), ("dh_fit_shape_cameras_device", lib.dh_fit_shape_cameras_device)):
        extra = (None,) if name.endswith("_device") else ()
        assert fn(ft, vp(frames), 2, 8, 8, None, vp(zeros), vp(zeros), None, 0, None, 1, None, vp(rec), *extra) == EINVAL
        assert "NULL camera table" in _err(lib) and name in _err(lib)
        assert fn(None, vp(frames), 2, 8, 8, None, vp(zeros), vp(zeros), None, 0, None, 1, None, vp(rec), *extra) == EINVAL
    assert (rec == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0
