"""The fit entry points without a GPU: exported and declared, the dh_fit_params / dh_fit_record layouts of the Python side equal
the C layout (a g++ program prints sizeof and offsetof from include/depthhead_hip.h), the defaults, and every refusal the header
lists answers DH_EINVAL with a message and leaves the output buffers untouched.  A fitter takes its device resources at its
first fit and every refusal is decided before, so none of this needs a device -- but for the model handles, which do: the
refusals that need a real model (the extent limit, a camera table of another length) are in tests/test_gpu_fit.py.  Two
refusals of the header are tested nowhere, because they take two devices: a model and a camera table that live on another
device than the fitter."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_fit_model_create", "dh_fit_model_destroy", "dh_fit_model_info", "dh_fit_params_default", "dh_fitter_create", "dh_fitter_destroy",
       "dh_fit_depth", "dh_fit_depth_cameras", "dh_fit_depth_device", "dh_fit_depth_cameras_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_fit_params size %zu\n", sizeof(dh_fit_params));
    F(dh_fit_params, coarse_iterations); F(dh_fit_params, iterations); F(dh_fit_params, gate); F(dh_fit_params, lambda);
    F(dh_fit_params, min_points); F(dh_fit_params, reserved0); F(dh_fit_params, reserved);
    printf("dh_fit_record size %zu\n", sizeof(dh_fit_record));
    F(dh_fit_record, points); F(dh_fit_record, steps); F(dh_fit_record, status); F(dh_fit_record, reserved); F(dh_fit_record, sum_r2_fixed);
    printf("consts %d %d %d %d %d\n", (int)DH_FIT_OK, (int)DH_FIT_FEW_POINTS, (int)DH_FIT_SINGULAR, (int)DH_FIT_MAX_POINTS, (int)DH_FIT_MAX_EXTENT);
    return 0;
}
"""


def test_fit_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    import depthhead_amd
    from depthhead_amd import fit
    for name in ("Fitter", "Model"):
        assert hasattr(depthhead_amd, name) and name in depthhead_amd.__all__, name
    for name in ("Model", "Fitter", "vertex_normals", "matrix_to_euler", "rms", "instances_from_poses"):
        assert callable(getattr(fit, name)), name
    assert (fit.FIT_OK, fit.FIT_FEW_POINTS, fit.FIT_SINGULAR) == (0, 1, 2)


def test_header_declares_every_fit_export():
    abi_kit.assert_header_equals_exports(NEW)


def test_layouts_match_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [int(v) for v in consts]
    assert consts == [0, 1, 2, _lib.FIT_MAX_POINTS, _lib.FIT_MAX_EXTENT] == [0, 1, 2, 32768, 4096]
    dt = _lib.FIT_RECORD_DTYPE
    assert c[("dh_fit_record", "size")] == dt.itemsize == 24
    for f in dt.names:
        assert c[("dh_fit_record", f)] == dt.fields[f][1], f
    assert c[("dh_fit_params", "size")] == C.sizeof(_lib.FitParams) == 56
    for f, _ in _lib.FitParams._fields_:
        assert c[("dh_fit_params", "lambda" if f == "lam" else f)] == getattr(_lib.FitParams, f).offset, f


def default_params(lib):
    p = _lib.FitParams()
    assert lib.dh_fit_params_default(C.byref(p)) == 0
    return p


def test_default_params(hip_lib):
    p = default_params(hip_lib)
    assert (p.coarse_iterations, p.iterations, list(p.gate), p.lam, p.min_points) == (6, 14, [120.0, 25.0], 1e-3, 16)
    assert (p.reserved0, list(p.reserved)) == (0, [0, 0])
    assert hip_lib.dh_fit_params_default(None) == EINVAL and "NULL" in _err(hip_lib)


def test_model_create_refusals(hip_lib):
    lib, vp = hip_lib, _lib.vp
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    m = np.array([[0, 0, -1], [0, 0, -1], [0, 0, -1]], np.float32)
    h = C.c_void_p(1234)
    assert lib.dh_fit_model_create(None, vp(m), 3, 0, C.byref(h)) == EINVAL and "NULL" in _err(lib) and h.value is None
    assert lib.dh_fit_model_create(vp(v), None, 3, 0, C.byref(h)) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_fit_model_create(vp(v), vp(m), 3, 0, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_fit_model_create(vp(v), vp(m), 0, 0, C.byref(h)) == EINVAL and "0 points" in _err(lib)
    assert lib.dh_fit_model_create(vp(v), vp(m), _lib.FIT_MAX_POINTS + 1, 0, C.byref(h)) == EINVAL and "32769 points" in _err(lib)
    for x in (np.nan, np.inf, -np.inf):
        w = v.copy(); w[2, 1] = x
        assert lib.dh_fit_model_create(vp(w), vp(m), 3, 0, C.byref(h)) == EINVAL and "point 2 is not finite" in _err(lib)
        w = m.copy(); w[1, 0] = x
        assert lib.dh_fit_model_create(vp(v), vp(w), 3, 0, C.byref(h)) == EINVAL and "normal 1 is not finite" in _err(lib)
    for ln in (0.0, 0.9899, 1.0100):                     # |m|^2 = 0, 0.9799, 1.0201: outside [0.98, 1.02]
        w = m.copy(); w[2] = (0, 0, -ln)
        assert lib.dh_fit_model_create(vp(v), vp(w), 3, 0, C.byref(h)) == EINVAL and "normal 2 has squared length" in _err(lib)
    assert h.value is None
    assert lib.dh_fit_model_destroy(None) == 0 and lib.dh_fitter_destroy(None) == 0
    assert lib.dh_fit_model_info(None, None, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_fitter_create(0, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_fitter_create(-1, C.byref(h)) == EINVAL and h.value is None


def test_fit_refusals_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    K = np.array([100, 0, 4, 0, 100, 4, 0, 0, 1], np.float32)
    frames = np.full((2, 8, 8), 800, np.uint16)
    out = np.full(2 * 64, 0xAB, np.uint8)
    rec = np.full(2 * 24, 0xCD, np.uint8)
    models = (C.c_void_p * 1)(None)
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value

    def inst(frame=0, model=0):
        a = np.zeros(1, _lib.RENDER_INSTANCE_DTYPE)
        a["frame"], a["mesh"], a["scale"] = frame, model, 1.0
        a["R"][0] = np.eye(3, dtype=np.float32).reshape(9)
        a["t"][0] = (0, 0, 800)
        return a

    def calls(f, ins, n, w, h, prm, fr=frames, o=out, r=rec, k=K, mdl=models):
        p = C.byref(prm) if prm is not None else None
        ni = 0 if ins is None else len(ins)
        yield "dh_fit_depth", lib.dh_fit_depth(f, vp(fr), n, w, h, vp(k), mdl, 1, vp(ins), ni, p, vp(o), vp(r))
        yield "dh_fit_depth_device", lib.dh_fit_depth_device(f, vp(fr), n, w, h, vp(k), mdl, 1, vp(ins), ni, p, vp(o), vp(r), None)

    def refused(what, *args, **kw):
        for name, rc in calls(*args, **kw):
            assert rc == EINVAL and what in _err(lib) and name in _err(lib), (name, rc, _err(lib))
        assert (out == 0xAB).all() and (rec == 0xCD).all()

    prm = default_params(lib)
    refused("NULL fitter", None, None, 2, 8, 8, prm)
    refused("NULL frames", ft, None, 2, 8, 8, prm, fr=None)
    refused("NULL output", ft, None, 2, 8, 8, prm, o=None)
    refused("NULL output", ft, None, 2, 8, 8, prm, r=None)
    refused("NULL K", ft, None, 2, 8, 8, prm, k=None)
    for n in (0, -1, 65536):
        refused("frames", ft, None, n, 8, 8, prm)
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, _lib.RENDER_MAX_SIZE + 1), (_lib.RENDER_MAX_SIZE + 1, 8)):
        refused("frame size", ft, None, 2, w, h, prm)
    refused("names frame 2 of 2", ft, inst(frame=2), 2, 8, 8, prm)
    refused("names frame 4294967295 of 2", ft, inst(frame=0xFFFFFFFF), 2, 8, 8, prm)
    refused("names model 1 of 1", ft, inst(model=1), 2, 8, 8, prm)
    refused("model 0 is NULL", ft, inst(), 2, 8, 8, prm)
    refused("NULL models", ft, inst(), 2, 8, 8, prm, mdl=None)
    for field, idx in (("R", 4), ("t", 2), ("scale", None)):
        for x in (np.nan, np.inf, -np.inf):
            a = inst()
            if idx is None:
                a[field][0] = x
            else:
                a[field][0, idx] = x
            refused("non-finite R, t or scale", ft, a, 2, 8, 8, prm)
    for idx, x, where in ((7, -2.5, "[1][2]"), (0, 1.011, "[0][0]"), (0, 0.989, "[0][0]"), (1, 0.021, "[0][1]"), (5, -0.021, "[1][2]")):
        a = inst()                                       # (R R^T - I) leaves DH_FIT_R_TOLERANCE = 0.02 at the named element first
        a["R"][0, idx] = x
        refused(f"not orthonormal: (R R^T){where}", ft, a, 2, 8, 8, prm)
    for idx, x in ((0, 1.0099), (0, 0.9901), (1, 0.0199)):    # within the tolerance: the next refusal (the model) answers
        a = inst()
        a["R"][0, idx] = x
        refused("model 0 is NULL", ft, a, 2, 8, 8, prm)
    for name, fn in (("dh_fit_depth", lib.dh_fit_depth),):
        assert fn(ft, vp(frames), 2, 8, 8, vp(K), models, 1, None, 1, None, vp(out), vp(rec)) == EINVAL and "NULL instances" in _err(lib)

    def with_params(**kw):
        p = default_params(lib)
        for k, v in kw.items():
            if k == "gate":
                p.gate[v[0]] = v[1]
            elif k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    refused("above 64", ft, None, 2, 8, 8, with_params(coarse_iterations=33, iterations=32))
    refused("above 64", ft, None, 2, 8, 8, with_params(coarse_iterations=0xFFFFFFFF, iterations=2))
    for g in (0, 1):
        for v in (0.0, -1.0, 4096.5, np.nan, np.inf):
            refused(f"gate[{g}]", ft, None, 2, 8, 8, with_params(gate=(g, v)))
    for v in (-1e-9, np.nan, np.inf):
        refused("lambda", ft, None, 2, 8, 8, with_params(lam=v))
    refused("min_points 5 below 6", ft, None, 2, 8, 8, with_params(min_points=5))
    refused("reserved", ft, None, 2, 8, 8, with_params(reserved0=1))
    refused("reserved", ft, None, 2, 8, 8, with_params(reserved=0))
    refused("reserved", ft, None, 2, 8, 8, with_params(reserved=1))
    for name, fn in (("dh_fit_depth_cameras", lib.dh_fit_depth_cameras), ("dh_fit_depth_cameras_device", lib.dh_fit_depth_cameras_device)):
        extra = (None,) if name.endswith("_device") else ()
        assert fn(ft, vp(frames), 2, 8, 8, None, models, 1, None, 0, None, vp(out), vp(rec), *extra) == EINVAL
        assert "NULL camera table" in _err(lib) and name in _err(lib)
        assert fn(None, vp(frames), 2, 8, 8, None, models, 1, None, 0, None, vp(out), vp(rec), *extra) == EINVAL
    # no instance: nothing to do, nothing written, no device touched
    for name, rc in calls(ft, None, 2, 8, 8, None):
        assert rc == 0, (name, _err(lib))
    assert (out == 0xAB).all() and (rec == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0
