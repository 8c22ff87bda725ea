"""The identification entry points without a GPU: exported and declared, the dh_ident_record and
dh_ident_params layouts of the Python side equal to the C layouts field for field (a g++ program prints sizeof and offsetof from
include/depthhead_hip.h), DH_IDENT_UNKNOWN equal to DH_SHAPE_SKIP, the defaults, and every refusal that is decided before a device
is touched, in the header's order, answering DH_EINVAL with a message and leaving the outputs untouched.  Where a call needs a
subject set that is not NULL it gets a block of bytes that reads as a set of 3 subjects on device 0 (or 1) whose memory is never
touched: every refusal made here comes before the set's models or basis are read.  The per-instance refusals of the host forms
need a real set: they are in tests/test_gpu_ident.py."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_fit_ident_params_default", "dh_fit_identify_subjects", "dh_fit_identify_subjects_cameras", "dh_fit_identify_subjects_device",
       "dh_fit_identify_subjects_cameras_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
static_assert(DH_IDENT_UNKNOWN == DH_SHAPE_SKIP, "subjects_out is a shape step's subjects");
int main() {
    printf("dh_ident_record size %zu\n", sizeof(dh_ident_record));
    F(dh_ident_record, status); F(dh_ident_record, best); F(dh_ident_record, second); F(dh_ident_record, eligible);
    F(dh_ident_record, points_best); F(dh_ident_record, points_second); F(dh_ident_record, sum_r2_best); F(dh_ident_record, sum_r2_second);
    printf("dh_ident_params size %zu\n", sizeof(dh_ident_params));
    F(dh_ident_params, iterations); F(dh_ident_params, min_points); F(dh_ident_params, gate); F(dh_ident_params, lambda);
    F(dh_ident_params, max_rms); F(dh_ident_params, min_ratio); F(dh_ident_params, reserved);
    printf("consts %u %u %u %u %u %u %u %u %g\n", DH_IDENT_OK, DH_IDENT_SKIPPED, DH_IDENT_NO_CANDIDATE, DH_IDENT_FAR, DH_IDENT_AMBIGUOUS, DH_IDENT_UNKNOWN,
           DH_SHAPE_SKIP, DH_IDENT_MAX_PAIRS, DH_IDENT_DEFAULT_MAX_RMS);
    return 0;
}
"""


def test_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    from depthhead_amd import fit
    for name in ("recognise_subjects", "ident_params"):
        assert callable(getattr(fit, name)), name
    assert callable(fit.Fitter.identify_subjects)
    assert fit.IDENT_RECORD_DTYPE is _lib.IDENT_RECORD_DTYPE and fit.IDENT_UNKNOWN == _lib.IDENT_UNKNOWN == _lib.SHAPE_SKIP == 0xFFFFFFFF
    assert (fit.IDENT_OK, fit.IDENT_SKIPPED, fit.IDENT_NO_CANDIDATE, fit.IDENT_FAR, fit.IDENT_AMBIGUOUS) == (0, 1, 2, 3, 4)


def test_header_and_exports_are_equal():
    abi_kit.assert_header_equals_exports(NEW)


def test_record_and_params_layouts_match_the_header(tmp_path, hip_lib):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [float(v) for v in consts]
    assert consts == [_lib.IDENT_OK, _lib.IDENT_SKIPPED, _lib.IDENT_NO_CANDIDATE, _lib.IDENT_FAR, _lib.IDENT_AMBIGUOUS, _lib.IDENT_UNKNOWN, _lib.SHAPE_SKIP,
                      _lib.IDENT_MAX_PAIRS, _lib.IDENT_DEFAULT_MAX_RMS] == [0, 1, 2, 3, 4, 0xFFFFFFFF, 0xFFFFFFFF, 1 << 22, 1.68]
    dt = _lib.IDENT_RECORD_DTYPE
    assert c[("dh_ident_record", "size")] == dt.itemsize == 40 == sum(dt.fields[f][0].itemsize for f in dt.names)        # no padding
    assert dt.names == ("status", "best", "second", "eligible", "points_best", "points_second", "sum_r2_best", "sum_r2_second")
    assert [dt.fields[f][1] for f in dt.names] == [0, 4, 8, 12, 16, 20, 24, 32]
    for f in dt.names:
        assert c[("dh_ident_record", f)] == dt.fields[f][1], f
    assert dt.fields["sum_r2_best"][0] == np.dtype("<i8") and dt.fields["sum_r2_second"][0] == np.dtype("<i8")
    P = _lib.IdentParams
    assert c[("dh_ident_params", "size")] == C.sizeof(P) == 64
    assert [n for n, _ in P._fields_] == ["iterations", "min_points", "gate", "lam", "max_rms", "min_ratio", "reserved"]
    for name, _ in P._fields_:
        assert c[("dh_ident_params", "lambda" if name == "lam" else name)] == getattr(P, name).offset, name


def test_the_defaults(hip_lib):
    p = _lib.IdentParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    assert hip_lib.dh_fit_ident_params_default(C.byref(p)) == 0
    assert (p.iterations, p.min_points, p.gate, p.lam, p.max_rms, p.min_ratio, p.reserved[0], p.reserved[1], p.reserved[2]) == \
        (4, 64, 25.0, 1e-3, 1.68, 1.0, 0, 0, 0)
    assert hip_lib.dh_fit_ident_params_default(None) == EINVAL and "NULL" in _err(hip_lib)
    from depthhead_amd import fit
    q = fit.ident_params(iterations=7, min_points=9, gate=30.0, lam=0.5, max_rms=np.inf, min_ratio=1.25)
    assert (q.iterations, q.min_points, q.gate, q.lam, q.max_rms, q.min_ratio) == (7, 9, 30.0, 0.5, np.inf, 1.25)


def stand_in_set(n_subjects=3, device=0):
    """256 bytes that read as a dh_fit_subjects of 642 points and n_subjects subjects on `device` with no memory (dh_api_fit.hip: int
    device; uint32 n, n_tris, n_subjects; ...) -- for the refusals that come before the set's models and basis are read."""
    block = np.zeros(256, np.uint8)
    block[0:4].view(np.int32)[:] = device
    block[4:16].view(np.uint32)[:] = (642, 1280, n_subjects)
    return block


def test_refusals_in_their_order_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    K = np.array([100, 0, 4, 0, 100, 4, 0, 0, 1], np.float32)
    frames = np.full((2, 8, 8), 800, np.uint16)
    inst = np.zeros(2, _lib.RENDER_INSTANCE_DTYPE)
    out = {name: np.full(512, 0xCD, np.uint8) for name in ("sub", "rec", "poses", "scores")}
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value
    good_set = stand_in_set()

    def calls(f=ft, fr=frames, st=good_set, sub=out["sub"], rec=out["rec"], n=2, w=8, h=8, k=K, ns=3, prm=None, instances=inst, ni=2, cams=False):
        """Every form with the same arguments: (name, return code, message)."""
        kind = "_cameras" if cams else ""
        args = (f, vp(fr), n, w, h, None if cams else vp(k), vp(st), vp(instances), C.c_uint32(ni), None, C.c_uint32(ns), None,
                C.byref(prm) if prm is not None else None, vp(sub), vp(rec), vp(out["poses"]), vp(out["scores"]))
        for name, extra in (("dh_fit_identify_subjects" + kind, ()), ("dh_fit_identify_subjects" + kind + "_device", (None,))):
            rc = getattr(lib, name)(*args, *extra)
            yield name, rc, _err(lib)

    def refused(text, both_kinds=False, **kw):
        for cams in ((False, True) if both_kinds else (False,)):
            for name, rc, msg in calls(cams=cams, **kw):
                assert rc == EINVAL and text in msg and name + ":" in msg, (name, rc, msg, text)
        for buf in out.values():
            assert (buf == 0xCD).all()

    # 1. the NULL pointers, each with every later refusal provoked as well
    later = dict(w=0, ns=0, prm=bad_params(gate=np.nan), instances=None, st=stand_in_set(device=1))
    refused("NULL fitter", both_kinds=True, f=None, **later)
    refused("NULL frames", both_kinds=True, fr=None, **later)
    refused("NULL subjects_out", both_kinds=True, sub=None, **later)
    refused("NULL records", both_kinds=True, rec=None, **later)
    refused("NULL subject set", both_kinds=True, **dict(later, st=None))
    # 2. the frames' refusals
    refused("n = 0, expected 1 .. 65535 frames", n=0, **later)
    for name, rc, msg in calls(**later):                                            # w = 0: the frame size (DH_EINVAL or DH_ESIZE, as dh_fit_shape* answers)
        assert rc != 0 and name + ":" in msg and "subject set lives" not in msg and "n_subjects" not in msg and "NaN" not in msg, msg
    refused("NULL K", **dict(later, k=None, w=8))
    for name, rc, msg in calls(cams=True, **dict(later, w=8)):
        assert rc == EINVAL and "NULL camera table" in msg, msg
    # 3. a set on another device, 4. n_subjects outside 1 .. S
    del later["w"], later["st"]
    refused("the subject set lives on device 1, the fitter on 0", st=stand_in_set(device=1), **later)
    del later["ns"]
    for ns in (0, 4, 0xFFFFFFFF):
        refused(f"n_subjects = {ns}, expected 1 .. 3", ns=ns, **later)
    # 5. the parameters, in the header's order, each with the later ones provoked as well
    del later["prm"]
    for kw in (dict(gate=np.nan), dict(lam=np.nan), dict(max_rms=np.nan), dict(min_ratio=np.nan)):
        refused("a value is NaN", prm=bad_params(**dict(dict(iterations=65, min_points=0), **kw)), **later)
    refused("iterations = 65 above 64", prm=bad_params(iterations=65, gate=0.0, lam=-1.0, min_points=5, max_rms=0.0, min_ratio=0.5, reserved=1), **later)
    for gate in (0.0, -1.0, 4096.5, np.inf):
        refused("gate", prm=bad_params(gate=gate, lam=-1.0, min_points=5, max_rms=0.0, min_ratio=0.5, reserved=1), **later)
    for lam in (-1e-9, np.inf):
        refused("lambda", prm=bad_params(lam=lam, min_points=5, max_rms=0.0, min_ratio=0.5, reserved=1), **later)
    refused("min_points 5 below 6", prm=bad_params(min_points=5, max_rms=0.0, min_ratio=0.5, reserved=1), **later)
    for rms in (0.0, -1.0, -np.inf):
        refused("max_rms", prm=bad_params(max_rms=rms, min_ratio=0.5, reserved=1), **later)
    for ratio in (0.999, 0.0, -np.inf):
        refused("min_ratio", prm=bad_params(min_ratio=ratio, reserved=1), **later)
    for word in range(3):
        p = bad_params()
        p.reserved[word] = 1
        refused("reserved", prm=p, **later)
    # 6. NULL instances, then 7. the pair limit
    refused("NULL instances", instances=None, ni=(1 << 22) + 1)
    refused(f"{(1 << 22) // 3 + 1} instances times 3 subjects exceed {1 << 22} pairs", ni=(1 << 22) // 3 + 1)
    # what is allowed: max_rms = +inf, iterations 0 and 64, no instances at all -- no error, nothing written
    for prm in (bad_params(max_rms=np.inf), bad_params(iterations=0), bad_params(iterations=64, min_points=6, gate=4096.0, lam=0.0)):
        for name, rc, msg in calls(prm=prm, ni=0, instances=None):
            assert rc == 0, (name, msg)
    for buf in out.values():
        assert (buf == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0


def bad_params(reserved=0, **kw):
    p = _lib.IdentParams()
    assert _lib.load().dh_fit_ident_params_default(C.byref(p)) == 0
    for name, value in kw.items():
        setattr(p, name, value)
    p.reserved[0] = reserved
    return p
