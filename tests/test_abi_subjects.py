"""The subject-set entry points without a GPU: exported and declared, the dh_subject_state layout of the
Python side equal to the C layout field for field (a g++ program prints sizeof and offsetof from include/depthhead_hip.h), and
every refusal that is decided before a device is touched, in the header's order, answers DH_EINVAL with a message and leaves the
outputs untouched.  A basis lives on a device, so where dh_fit_subjects_create needs a handle that is not NULL it gets a block of
zeros (a basis of 0 points on device 0): the basis is the LAST thing the call looks at, so every refusal before it is reached
with it, and the call ends at "the basis is one of 0 points" before anything is allocated.  The refusals that need a real set are
in tests/test_gpu_subjects.py."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_fit_subjects_create", "dh_fit_subjects_destroy", "dh_fit_subjects_info", "dh_fit_subjects_model", "dh_fit_subjects_set_coeffs",
       "dh_fit_subjects_state", "dh_fit_subjects_read", "dh_fit_subjects_update", "dh_fit_subjects_update_device", "dh_fit_shape_subjects", "dh_fit_shape_subjects_cameras",
       "dh_fit_shape_subjects_device", "dh_fit_shape_subjects_cameras_device", "dh_fit_depth_carried_device", "dh_fit_depth_cameras_carried_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_subject_state size %zu\n", sizeof(dh_subject_state));
    F(dh_subject_state, coeffs); F(dh_subject_state, applied); F(dh_subject_state, rejected); F(dh_subject_state, flags); F(dh_subject_state, zero_normals);
    printf("consts %u %u %u\n", DH_SUBJECTS_MAX_TRIS, DH_SUBJECT_CLAMPED, DH_SUBJECT_NONFINITE);
    return 0;
}
"""


def test_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    import depthhead_amd
    from depthhead_amd import fit
    assert hasattr(depthhead_amd, "Subjects") and "Subjects" in depthhead_amd.__all__
    for name in ("Subjects", "adapt_subjects"):
        assert callable(getattr(fit, name)), name
    assert callable(fit.Fitter.shape_step_subjects)
    assert fit.SUBJECT_STATE_DTYPE is _lib.SUBJECT_STATE_DTYPE
    assert (fit.SUBJECT_CLAMPED, fit.SUBJECT_NONFINITE) == (1, 2)


def test_header_and_exports_are_equal():
    abi_kit.assert_header_equals_exports(NEW)


def test_state_layout_matches_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [int(v) for v in consts]
    assert consts == [_lib.SUBJECTS_MAX_TRIS, _lib.SUBJECT_CLAMPED, _lib.SUBJECT_NONFINITE] == [131072, 1, 2]
    dt = _lib.SUBJECT_STATE_DTYPE
    assert c[("dh_subject_state", "size")] == dt.itemsize == 80 == sum(dt.fields[f][0].itemsize for f in dt.names)      # no padding
    assert dt.names == ("coeffs", "applied", "rejected", "flags", "zero_normals")
    assert [dt.fields[f][1] for f in dt.names] == [0, 64, 68, 72, 76]
    for f in dt.names:
        assert c[("dh_subject_state", f)] == dt.fields[f][1], f
    assert dt.fields["coeffs"][0].shape == (8,) and dt.fields["coeffs"][0].base == np.dtype("<f8")


TETRA_V = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float32)
TETRA_T = np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.uint32)


def test_create_refusals_in_their_order(hip_lib):
    lib, vp = hip_lib, _lib.vp
    # a basis handle that is not NULL: 0 points on device 0.  (dh_api_fit.hip pins sizeof(dh_fit_basis) <= 256 with a static_assert, so
    # the library never reads past this block; its device memory is never touched before the call has ended)
    zeros = np.zeros(256, np.uint8)

    def create(v=TETRA_V, n=4, t=TETRA_T, nt=4, basis=zeros, ns=1, mc=0.5, device=0, out=True):
        h = C.c_void_p(1234)
        rc = lib.dh_fit_subjects_create(vp(v), C.c_uint32(n), vp(t), C.c_uint32(nt), vp(basis), C.c_uint32(ns), C.c_double(mc), device,
                                        C.byref(h) if out else None)
        assert rc == EINVAL and "dh_fit_subjects_create" in _err(lib), (rc, _err(lib))
        assert not out or h.value is None
        return _err(lib)

    assert "NULL" in create(out=False)
    assert "NULL" in create(v=None) and "NULL" in create(t=None) and "NULL" in create(basis=None)
    # each refusal with every LATER one provoked as well: the earlier one is what is reported
    later = dict(nt=0, ns=0, mc=0.0, device=-1)
    assert "0 points" in create(n=0, **later) and "32769 points" in create(n=_lib.FIT_MAX_POINTS + 1, **later)
    del later["nt"]
    assert "0 triangles" in create(nt=0, **later) and "131073 triangles" in create(nt=131073, **later)
    del later["ns"]
    for ns in (0, 257, 0xFFFFFFFF):
        assert f"n_subjects = {ns}" in create(ns=ns, **later)
    del later["mc"]
    for mc in (0.0, -0.5, np.nan, np.inf):
        assert "max_coeff" in create(mc=mc, **later)
    assert "device -1" in create(device=-1, v=np.full((4, 3), np.nan, np.float32))
    for x in (np.nan, np.inf, -np.inf):
        v = TETRA_V.copy(); v[2, 1] = x
        bad_t = TETRA_T.copy(); bad_t[0, 0] = 4
        assert "vertex 2 is not finite" in create(v=v, t=bad_t)
    for idx in (4, 0xFFFFFFFF):
        t = TETRA_T.copy(); t[2, 1] = idx
        flat = np.zeros((4, 3), np.float32)
        assert "triangle 2 names a vertex" in create(t=t, v=flat)
    line = np.array([(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3)], np.float32)
    assert "vertex 0 of the base mesh has a zero normal" in create(v=line)
    five = np.concatenate([TETRA_V, [[5, 5, 5]]]).astype(np.float32)
    assert "vertex 4 of the base mesh has a zero normal" in create(v=five, n=5)
    assert "the basis is one of 0 points, the mesh has 4" in create()


def test_the_other_calls_refuse_null(hip_lib):
    lib, vp = hip_lib, _lib.vp
    buf = np.full(512, 0xCD, np.uint8)
    assert lib.dh_fit_subjects_destroy(None) == 0
    assert lib.dh_fit_subjects_info(None, None, None, None, None, None, None) == EINVAL and "NULL subject set" in _err(lib)
    h = C.c_void_p(1234)
    assert lib.dh_fit_subjects_model(None, 0, C.byref(h)) == EINVAL and "NULL" in _err(lib) and h.value == 1234
    assert lib.dh_fit_subjects_set_coeffs(None, 0, 1, vp(buf)) == EINVAL and "NULL subject set" in _err(lib)
    assert lib.dh_fit_subjects_state(None, vp(buf)) == EINVAL and "NULL subject set" in _err(lib)
    assert lib.dh_fit_subjects_read(None, 0, vp(buf), vp(buf)) == EINVAL and "NULL subject set" in _err(lib)
    assert lib.dh_fit_subjects_update(None, vp(buf)) == EINVAL and "NULL subject set" in _err(lib)
    assert lib.dh_fit_subjects_update_device(None, vp(buf), None) == EINVAL and "NULL subject set" in _err(lib)
    assert (buf == 0xCD).all()


def test_shape_step_and_carried_fit_refusals_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    K = np.array([100, 0, 4, 0, 100, 4, 0, 0, 1], np.float32)
    frames = np.full((2, 8, 8), 800, np.uint16)
    rec = np.full(2 * 88, 0xCD, np.uint8)
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value

    def calls(f, fr, r, k=K, cams=False):
        host = (f, vp(fr), 2, 8, 8, None if cams else vp(k), None, None, 0, None, 1, None, None, vp(r))
        kind = "_cameras" if cams else ""
        yield "dh_fit_shape_subjects" + kind, getattr(lib, "dh_fit_shape_subjects" + kind)(*host)
        yield "dh_fit_shape_subjects" + kind + "_device", getattr(lib, "dh_fit_shape_subjects" + kind + "_device")(*host, None)

    for what, args in (("NULL fitter", (None, frames, rec)), ("NULL frames", (ft, None, rec)), ("NULL records", (ft, frames, None)),
                       ("NULL subject set", (ft, frames, rec))):
        for cams in (False, True):
            for name, rc in calls(*args, cams=cams):
                assert rc == EINVAL and what in _err(lib) and name in _err(lib), (name, rc, _err(lib))
    assert (rec == 0xCD).all()
    # the carried fit: its own refusal, then dh_fit_depth_device's
    inst = np.zeros(1, _lib.RENDER_INSTANCE_DTYPE)
    inst["scale"], inst["R"][0], inst["t"][0] = 1.0, np.eye(3, dtype=np.float32).reshape(9), (0, 0, 800)
    out = np.full(64, 0xCD, np.uint8)
    models = (C.c_void_p * 1)(None)
    for name, karg in (("dh_fit_depth_carried_device", vp(K)), ("dh_fit_depth_cameras_carried_device", None)):
        fn = getattr(lib, name)
        assert fn(ft, vp(frames), 2, 8, 8, karg, models, 1, vp(inst), 1, None, None, vp(out), vp(rec), None) == EINVAL
        assert "NULL carried instances" in _err(lib) and name in _err(lib)
        assert fn(None, vp(frames), 2, 8, 8, karg, models, 1, vp(inst), 1, vp(out), None, vp(out), vp(rec), None) == EINVAL
        assert "NULL fitter" in _err(lib) and name in _err(lib)
        if karg is not None:
            assert fn(ft, vp(frames), 2, 8, 8, karg, models, 1, vp(inst), 1, vp(out), None, vp(out), vp(rec), None) == EINVAL
            assert "model 0 is NULL" in _err(lib) and name in _err(lib)
    assert (rec == 0xCD).all() and (out == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0
