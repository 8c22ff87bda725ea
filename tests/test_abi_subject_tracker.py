"""The subject fit tracker's entry points without a GPU: exported and declared, the dh_subject_track_params /
_state / _record layouts of the Python side and of the restatement equal the C layout (a g++ program prints sizeof and offsetof
from include/depthhead_hip.h: 24, 92 and 160 bytes, no padding), the defaults, and every refusal that can be reached without a
device, in the header's order, answers DH_EINVAL with a message and leaves its outputs untouched.  A camera table, a set and a
model need a device, so a tracker cannot exist here: the refusals past the NULL handles (the ident params, the reserved words of
the dh_subject_track_params, devices, point counts, extents, pairs) and those that need a tracker are in
tests/test_gpu_subject_tracker.py."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_subject_track_params_default", "dh_subject_fit_tracker_create", "dh_subject_fit_tracker_destroy", "dh_subject_fit_tracker_reset",
       "dh_subject_fit_tracker_state", "dh_subject_fit_tracker_info", "dh_subject_fit_tracker_set_enrolled", "dh_subject_fit_tracker_bind",
       "dh_subject_fit_tracker_step_poses", "dh_subject_fit_tracker_step_poses_device", "dh_subject_fit_tracker_step",
       "dh_subject_fit_tracker_step_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_subject_track_params size %zu\n", sizeof(dh_subject_track_params));
    F(dh_subject_track_params, retry); F(dh_subject_track_params, max_tries); F(dh_subject_track_params, reserved);
    printf("dh_subject_track_state size %zu\n", sizeof(dh_subject_track_state));
    F(dh_subject_track_state, fit); F(dh_subject_track_state, subject); F(dh_subject_track_state, wait); F(dh_subject_track_state, tries);
    F(dh_subject_track_state, bound_age);
    printf("dh_subject_track_record size %zu\n", sizeof(dh_subject_track_record));
    F(dh_subject_track_record, track); F(dh_subject_track_record, ident); F(dh_subject_track_record, subject); F(dh_subject_track_record, model);
    F(dh_subject_track_record, identified); F(dh_subject_track_record, tries);
    return 0;
}
"""


def test_subject_tracker_entry_points_are_exported_and_declared(hip_lib):
    text = abi_kit.header()
    abi_kit.assert_exported(hip_lib, NEW)
    abi_kit.assert_header_equals_exports(NEW)
    import depthhead_amd
    from depthhead_amd import fit
    assert hasattr(depthhead_amd, "SubjectFitTracker") and "SubjectFitTracker" in depthhead_amd.__all__
    for name in ("step", "step_poses", "step_device", "reset", "state", "info", "bind", "set_enrolled"):
        assert callable(getattr(fit.SubjectFitTracker, name)), name
    assert callable(fit.subject_track_params)
    assert "PARITY UNPINNED" in text[text.index("following each tracked head with its own subject's model"):]
    from depthhead_amd import build
    assert "k_subject_track.hip" in build.SOURCES


def test_layouts_match_the_header(tmp_path):
    c, _ = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    import subject_track_ref as stf
    for name, dt, ref, size in (("dh_subject_track_state", _lib.SUBJECT_TRACK_STATE_DTYPE, stf.STATE, 92),
                                ("dh_subject_track_record", _lib.SUBJECT_TRACK_RECORD_DTYPE, stf.RECORD, 160)):
        assert c[(name, "size")] == dt.itemsize == ref.itemsize == size
        assert dt.names == ref.names
        for f in dt.names:
            assert c[(name, f)] == dt.fields[f][1] == ref.fields[f][1], (name, f)
        # no padding: the fields fill the record
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == size
    assert c[("dh_subject_track_params", "size")] == C.sizeof(_lib.SubjectTrackParams) == 24
    for f, _ in _lib.SubjectTrackParams._fields_:
        assert c[("dh_subject_track_params", f)] == getattr(_lib.SubjectTrackParams, f).offset, f
    assert _lib.SUBJECT_TRACK_STATE_DTYPE.fields["fit"][0] == _lib.FIT_TRACK_STATE_DTYPE
    assert _lib.SUBJECT_TRACK_RECORD_DTYPE.fields["track"][0] == _lib.FIT_TRACK_RECORD_DTYPE
    assert _lib.SUBJECT_TRACK_RECORD_DTYPE.fields["ident"][0] == _lib.IDENT_RECORD_DTYPE


def test_default_params(hip_lib):
    p = _lib.SubjectTrackParams()
    p.retry, p.max_tries, p.reserved[0], p.reserved[1] = 77, 77, 77, 77
    assert hip_lib.dh_subject_track_params_default(C.byref(p)) == 0
    assert (p.retry, p.max_tries, list(p.reserved)) == (4, 4, [0, 0])
    assert hip_lib.dh_subject_track_params_default(None) == EINVAL and "NULL" in _err(hip_lib)
    import subject_track_ref as stf
    assert stf.params() == {"retry": 4, "max_tries": 4}
    from depthhead_amd import fit
    q = fit.subject_track_params(retry=0, max_tries=9)
    assert (q.retry, q.max_tries, list(q.reserved)) == (0, 9, [0, 0])


def test_create_refusals_in_the_headers_order(hip_lib):
    """Every refusal before the handles are looked at, each with all LATER faults present too: the earlier one answers."""
    lib = hip_lib
    h = C.c_void_p(1234)
    track = _lib.FitTrackParams()
    assert lib.dh_fit_track_params_default(C.byref(track)) == 0

    def create(prm=None, flags=0, scale=1.0, out=h, cams=None, st=None, model=None, ident=None, sub=None):
        return lib.dh_subject_fit_tracker_create(cams, st, model, C.c_float(scale), C.c_uint32(flags), _lib.ref(prm), _lib.ref(ident), _lib.ref(sub),
                                                 None, C.byref(out) if out is not None else None)

    def with_params(**kw):
        p = _lib.FitTrackParams()
        assert lib.dh_fit_track_params_default(C.byref(p)) == 0
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    bad_ident = _lib.IdentParams()
    assert lib.dh_fit_ident_params_default(C.byref(bad_ident)) == 0
    bad_ident.iterations = 65
    bad_sub = _lib.SubjectTrackParams()
    bad_sub.reserved[1] = 1
    later = dict(ident=bad_ident, sub=bad_sub)
    assert create(out=None) == EINVAL and "NULL" in _err(lib)
    chain = [(dict(flags=2), "unknown flags"), (dict(scale=np.nan), "scale is not finite"),
             (dict(prm=with_params(iterations_tracked=65)), "iterations_tracked 65 above 64"), (dict(prm=with_params(rms_max=0.0)), "rms_max"),
             (dict(prm=with_params(max_jump=np.nan)), "max_jump"), (dict(prm=with_params(conf_den=0)), "confidence"),
             (dict(prm=with_params(reserved=1)), "reserved word of the params")]
    for i, (kw, what) in enumerate(chain):
        # this fault with every later fault of the chain's parameters where they do not collide, and the NULL handles and bad params after them
        merged = dict(later)
        if "prm" not in kw:
            merged["prm"] = with_params(iterations_tracked=65, rms_max=0.0, conf_den=0)
        if "scale" not in kw and i == 0:
            merged["scale"] = np.inf
        merged.update(kw)
        assert create(**merged) == EINVAL and what in _err(lib) and "dh_subject_fit_tracker_create" in _err(lib), (what, _err(lib))
        assert h.value is None
    assert create(**later) == EINVAL and "NULL camera table" in _err(lib)
    assert create(cams=C.c_void_p(8), **later) == EINVAL and "NULL subject set" in _err(lib)
    assert create(cams=C.c_void_p(8), st=C.c_void_p(8), **later) == EINVAL and "NULL model" in _err(lib)      # (no handle is read before all three are there)
    for scale in (np.inf, -np.inf):
        assert create(scale=scale) == EINVAL and "scale is not finite" in _err(lib)
    for flags in (0x80000000, 3):
        assert create(flags=flags) == EINVAL and "unknown flags" in _err(lib)
    # within range: the next refusal (the camera table) answers
    for p in (with_params(iterations_tracked=64), with_params(rms_max=4096.0), with_params(conf_num=50)):
        assert create(p) == EINVAL and "NULL camera table" in _err(lib)
    assert create(flags=1) == EINVAL and "NULL camera table" in _err(lib) and h.value is None


def test_refusals_without_a_tracker_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    frames = np.full((1, 8, 8), 800, np.uint16)
    poses, sup = np.zeros(1, _lib.POSE_DTYPE), np.zeros(1, _lib.SUPPORT_DTYPE)
    rec = np.full(160, 0xCD, np.uint8)
    st = np.full(92, 0xAB, np.uint8)
    n, s, g = C.c_int(-7), C.c_uint32(77), C.c_uint32(77)
    assert lib.dh_subject_fit_tracker_step_poses(None, vp(frames), 8, 8, None, vp(poses), vp(sup), None, vp(rec)) == EINVAL
    assert "NULL tracker" in _err(lib) and "dh_subject_fit_tracker_step_poses" in _err(lib)
    assert lib.dh_subject_fit_tracker_step_poses_device(None, vp(frames), 8, 8, None, vp(poses), vp(sup), None, vp(rec), None) == EINVAL
    assert "NULL tracker" in _err(lib) and "dh_subject_fit_tracker_step_poses_device" in _err(lib)
    assert lib.dh_subject_fit_tracker_step(None, None, vp(frames), 8, 8, None, 30, None, vp(poses), vp(sup), vp(rec)) == EINVAL
    assert "NULL predictor" in _err(lib)
    assert lib.dh_subject_fit_tracker_step_device(None, None, vp(frames), 8, 8, None, 30, None, vp(poses), vp(sup), vp(rec), None) == EINVAL
    assert "NULL predictor" in _err(lib)
    assert lib.dh_subject_fit_tracker_step(C.c_void_p(8), None, vp(frames), 8, 8, None, 30, None, vp(poses), vp(sup), vp(rec)) == EINVAL
    assert "NULL tracker" in _err(lib)
    assert lib.dh_subject_fit_tracker_step_device(C.c_void_p(8), None, vp(frames), 8, 8, None, 30, None, vp(poses), vp(sup), vp(rec), None) == EINVAL
    assert "NULL tracker" in _err(lib)
    assert lib.dh_subject_fit_tracker_reset(None, -1, None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_subject_fit_tracker_state(None, vp(st)) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_subject_fit_tracker_info(None, C.byref(n), C.byref(s), C.byref(g)) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_subject_fit_tracker_bind(None, 0, C.c_uint32(0), None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_subject_fit_tracker_set_enrolled(None, None, None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_subject_fit_tracker_destroy(None) == 0
    assert (rec == 0xCD).all() and (st == 0xAB).all() and not poses.tobytes().strip(b"\0") and not sup.tobytes().strip(b"\0")
    assert (n.value, s.value, g.value) == (-7, 77, 77)
