"""The surface entry points without a GPU: exported and declared, the dh_surface_record and dh_surface_params
layouts of the Python side equal to the C layouts field for field (a g++ program prints sizeof and offsetof from
include/depthhead_hip.h), and every refusal that is decided before a device is touched, in the header's order, answers DH_EINVAL
with a message and leaves the outputs untouched.  Where dh_fit_subjects_create_surface needs a basis handle that is not NULL it
gets a block of bytes that reads as a basis of the mesh's point count on device 0 whose memory is never touched: the two refusals
the surface adds come after the basis's, so they are reached with it, and the call ends before anything is allocated.  A set
of either kind cannot be made without a device: the surface calls refused on an ordinary set, and the refusals that need a real
surface set, are in tests/test_gpu_surface.py."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_fit_subjects_create_surface", "dh_fit_subjects_set_offsets", "dh_fit_subjects_read_offsets", "dh_fit_surface_params_default",
       "dh_fit_surface_subjects", "dh_fit_surface_subjects_cameras", "dh_fit_surface_subjects_device", "dh_fit_surface_subjects_cameras_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_surface_record size %zu\n", sizeof(dh_surface_record));
    F(dh_surface_record, status); F(dh_surface_record, points); F(dh_surface_record, instances); F(dh_surface_record, observed);
    F(dh_surface_record, clamped); F(dh_surface_record, rejected); F(dh_surface_record, sum_r2_fixed); F(dh_surface_record, max_abs);
    printf("dh_surface_params size %zu\n", sizeof(dh_surface_params));
    F(dh_surface_params, gate); F(dh_surface_params, min_cos2); F(dh_surface_params, mu); F(dh_surface_params, eps);
    F(dh_surface_params, min_count); F(dh_surface_params, min_points); F(dh_surface_params, iterations); F(dh_surface_params, reserved0);
    F(dh_surface_params, reserved);
    printf("consts %u %u %g %g %u %u\n", DH_SURFACE_OK, DH_SURFACE_FEW_POINTS, DH_SURFACE_MAX_OFFSET, DH_SURFACE_MAX_SCALE, DH_SURFACE_MAX_CELLS,
           DH_SURFACE_MAX_ITERATIONS);
    return 0;
}
"""


def test_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    from depthhead_amd import fit
    for name in ("refine_subjects", "surface_params"):
        assert callable(getattr(fit, name)), name
    assert callable(fit.Fitter.surface_step_subjects) and callable(fit.Subjects.offsets) and callable(fit.Subjects.set_offsets)
    assert fit.SURFACE_RECORD_DTYPE is _lib.SURFACE_RECORD_DTYPE
    assert (fit.SURFACE_OK, fit.SURFACE_FEW_POINTS) == (0, 1)


def test_header_and_exports_are_equal():
    abi_kit.assert_header_equals_exports(NEW)


def test_record_and_params_layouts_match_the_header(tmp_path, hip_lib):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [float(v) for v in consts]
    assert consts == [_lib.SURFACE_OK, _lib.SURFACE_FEW_POINTS, _lib.SURFACE_MAX_OFFSET, _lib.SURFACE_MAX_SCALE, _lib.SURFACE_MAX_CELLS,
                      _lib.SURFACE_MAX_ITERATIONS] == [0, 1, 64, 64, 1 << 22, 256]
    dt = _lib.SURFACE_RECORD_DTYPE
    assert c[("dh_surface_record", "size")] == dt.itemsize == 40 == sum(dt.fields[f][0].itemsize for f in dt.names)      # no padding
    assert dt.names == ("status", "points", "instances", "observed", "clamped", "rejected", "sum_r2_fixed", "max_abs")
    assert [dt.fields[f][1] for f in dt.names] == [0, 4, 8, 12, 16, 20, 24, 32]
    for f in dt.names:
        assert c[("dh_surface_record", f)] == dt.fields[f][1], f
    assert dt.fields["sum_r2_fixed"][0] == np.dtype("<i8") and dt.fields["max_abs"][0] == np.dtype("<f8")
    P = _lib.SurfaceParams
    assert c[("dh_surface_params", "size")] == C.sizeof(P) == 64
    assert [n for n, _ in P._fields_] == ["gate", "min_cos2", "mu", "eps", "min_count", "min_points", "iterations", "reserved0", "reserved"]
    for name, _ in P._fields_:
        assert c[("dh_surface_params", name)] == getattr(P, name).offset, name
    # the defaults
    p = P()
    assert hip_lib.dh_fit_surface_params_default(C.byref(p)) == 0
    assert (p.gate, p.min_cos2, p.mu, p.eps, p.min_count, p.min_points, p.iterations, p.reserved0, p.reserved[0], p.reserved[1]) == \
        (25.0, 0.25, 0.5, 0.05, 2, 64, 32, 0, 0, 0)
    assert hip_lib.dh_fit_surface_params_default(None) == EINVAL and "NULL" in _err(hip_lib)


TETRA_V = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float32)
TETRA_T = np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.uint32)


def stand_in_basis(n, k=1):
    """256 bytes that read as a dh_fit_basis of n points and k fields on device 0 with largest 0 and no memory (dh_api_fit.hip: int
    device; uint32 n, k; double largest; the buffer) -- for refusals that come after the basis's own."""
    block = np.zeros(256, np.uint8)
    block[4:12].view(np.uint32)[:] = (n, k)
    return block


def test_create_refusals_in_their_order(hip_lib):
    lib, vp = hip_lib, _lib.vp

    def create(v=TETRA_V, n=4, t=TETRA_T, nt=4, basis=None, ns=1, mc=0.5, mo=8.0, device=0, out=True, null_basis=False):
        h = C.c_void_p(1234)
        b = None if null_basis else (stand_in_basis(n) if basis is None else basis)
        rc = lib.dh_fit_subjects_create_surface(vp(v), C.c_uint32(n), vp(t), C.c_uint32(nt), vp(b), C.c_uint32(ns), C.c_double(mc), C.c_double(mo),
                                                device, C.byref(h) if out else None)
        assert rc == EINVAL and "dh_fit_subjects_create_surface" in _err(lib), (rc, _err(lib))
        assert not out or h.value is None
        return _err(lib)

    assert "NULL" in create(out=False)
    assert "NULL" in create(v=None) and "NULL" in create(t=None) and "NULL" in create(null_basis=True)
    # dh_fit_subjects_create's refusals in its order, each with every LATER one provoked as well -- the surface's own among them
    later = dict(nt=0, ns=0, mc=0.0, mo=0.0, device=-1)
    assert "0 points" in create(n=0, **later) and "32769 points" in create(n=_lib.FIT_MAX_POINTS + 1, **later)
    del later["nt"]
    assert "0 triangles" in create(nt=0, **later) and "131073 triangles" in create(nt=131073, **later)
    del later["ns"]
    for ns in (0, 257, 0xFFFFFFFF):
        assert f"n_subjects = {ns}" in create(ns=ns, **later)
    del later["mc"]
    for mc in (0.0, -0.5, np.nan, np.inf):
        assert "max_coeff" in create(mc=mc, **later)
    assert "device -1" in create(device=-1, mo=0.0, v=np.full((4, 3), np.nan, np.float32))
    v = TETRA_V.copy(); v[2, 1] = np.nan
    assert "vertex 2 is not finite" in create(v=v, mo=0.0)
    t = TETRA_T.copy(); t[2, 1] = 4
    assert "triangle 2 names a vertex" in create(t=t, mo=0.0)
    line = np.array([(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3)], np.float32)
    assert "vertex 0 of the base mesh has a zero normal" in create(v=line, mo=0.0)
    assert "the basis is one of 0 points, the mesh has 4" in create(basis=np.zeros(256, np.uint8), mo=0.0)
    other = stand_in_basis(4)
    other[0:4].view(np.int32)[:] = 1
    assert "the basis lives on device 1" in create(basis=other, mo=0.0)
    # then the surface's own: max_offset, then the cell limit
    big_n = (_lib.SURFACE_MAX_CELLS // 256) + 1                                     # 256 subjects of this many vertices: one row too many
    for mo in (0.0, -1.0, 64.5, np.nan, np.inf):
        assert "max_offset" in create(mo=mo, ns=256, n=4)
    fan_t = np.array([(i, (i + 1) % big_n, (i + 2) % big_n) for i in range(big_n)], np.uint32)
    wavy = np.stack([np.cos(np.arange(big_n) * 0.001) * 50, np.sin(np.arange(big_n) * 0.001) * 50, 3.0 * np.sin(np.arange(big_n) * 1.7)], axis=1).astype(np.float32)
    msg = create(v=wavy, n=big_n, t=fan_t, nt=big_n, ns=256, mo=np.nan)
    assert "max_offset" in msg, msg
    msg = create(v=wavy, n=big_n, t=fan_t, nt=big_n, ns=256)
    assert f"256 subjects of {big_n} vertices exceed {_lib.SURFACE_MAX_CELLS} cells" in msg, msg


def test_the_other_calls_refuse_null(hip_lib):
    lib, vp = hip_lib, _lib.vp
    buf = np.full(512, 0xCD, np.uint8)
    assert lib.dh_fit_subjects_set_offsets(None, 0, vp(buf)) == EINVAL and "NULL subject set" in _err(lib)
    assert lib.dh_fit_subjects_read_offsets(None, 0, vp(buf), vp(buf)) == EINVAL and "NULL subject set" in _err(lib)
    assert (buf == 0xCD).all()


def test_step_refusals_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    K = np.array([100, 0, 4, 0, 100, 4, 0, 0, 1], np.float32)
    frames = np.full((2, 8, 8), 800, np.uint16)
    rec = np.full(2 * 40, 0xCD, np.uint8)
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value

    def calls(f, fr, r, k=K, cams=False):
        host = (f, vp(fr), 2, 8, 8, None if cams else vp(k), None, None, 0, None, 1, None, None, vp(r))
        kind = "_cameras" if cams else ""
        yield "dh_fit_surface_subjects" + kind, getattr(lib, "dh_fit_surface_subjects" + kind)(*host)
        yield "dh_fit_surface_subjects" + kind + "_device", getattr(lib, "dh_fit_surface_subjects" + kind + "_device")(*host, None)

    for what, args in (("NULL fitter", (None, frames, rec)), ("NULL frames", (ft, None, rec)), ("NULL records", (ft, frames, None)),
                       ("NULL subject set", (ft, frames, rec))):
        for cams in (False, True):
            for name, rc in calls(*args, cams=cams):
                assert rc == EINVAL and what in _err(lib) and name in _err(lib), (name, rc, _err(lib))
    assert (rec == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0
