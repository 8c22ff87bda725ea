"""The fit tracker's entry points without a GPU: exported and declared, the dh_fit_track_params / _state / _record layouts of the
Python side equal the C layout (a g++ program prints sizeof and offsetof from include/depthhead_hip.h), the defaults, the
angle table against numpy within 1 ulp, and every refusal that can be reached without a device answers DH_EINVAL with a message
and leaves its outputs untouched.  A camera table and a model need a device, so a tracker cannot exist here: creation's
parameter refusals are decided before the table and the model are looked at, and the refusals that need a tracker (the step's
NULL arguments, frame size and dh_fit_params, reset's camera index, a model too large for `scale`) are in
tests/test_gpu_fit_tracker.py."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_fit_track_params_default", "dh_fit_tracker_angles", "dh_fit_tracker_create", "dh_fit_tracker_destroy", "dh_fit_tracker_reset",
       "dh_fit_tracker_state", "dh_fit_tracker_step_poses", "dh_fit_tracker_step_poses_device", "dh_fit_tracker_step",
       "dh_fit_tracker_step_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_fit_track_params size %zu\n", sizeof(dh_fit_track_params));
    F(dh_fit_track_params, iterations_tracked); F(dh_fit_track_params, keep_points); F(dh_fit_track_params, rms_max);
    F(dh_fit_track_params, max_jump); F(dh_fit_track_params, conf_num); F(dh_fit_track_params, conf_den);
    F(dh_fit_track_params, min_windows); F(dh_fit_track_params, max_coast); F(dh_fit_track_params, reserved);
    printf("dh_fit_track_state size %zu\n", sizeof(dh_fit_track_state));
    F(dh_fit_track_state, R); F(dh_fit_track_state, t); F(dh_fit_track_state, t_prev); F(dh_fit_track_state, tracked);
    F(dh_fit_track_state, have_prev); F(dh_fit_track_state, age); F(dh_fit_track_state, lost);
    printf("dh_fit_track_record size %zu\n", sizeof(dh_fit_track_record));
    F(dh_fit_track_record, instance); F(dh_fit_track_record, fit); F(dh_fit_track_record, status); F(dh_fit_track_record, age);
    F(dh_fit_track_record, lost); F(dh_fit_track_record, reserved);
    printf("consts %u %u %u %u %u %u %u %u %u %u %d\n", DH_FIT_TRACK_NONE, DH_FIT_TRACK_FITTED, DH_FIT_TRACK_CARRIED, DH_FIT_TRACK_REJECTED,
           DH_FIT_TRACK_ABSENT, DH_FIT_TRACK_BAD_STATUS, DH_FIT_TRACK_BAD_POINTS, DH_FIT_TRACK_BAD_RMS, DH_FIT_TRACK_BAD_JUMP,
           DH_FIT_TRACK_MOTION, DH_FIT_TRACK_ANGLES);
    return 0;
}
"""


def test_fit_tracker_entry_points_are_exported_and_declared(hip_lib):
    text = abi_kit.header()
    abi_kit.assert_exported(hip_lib, NEW)
    abi_kit.assert_header_equals_exports(NEW)
    import depthhead_amd
    from depthhead_amd import fit
    assert hasattr(depthhead_amd, "FitTracker") and "FitTracker" in depthhead_amd.__all__
    for name in ("step", "step_poses", "step_device", "reset", "state", "angles"):
        assert callable(getattr(fit.FitTracker, name)), name
    assert fit.FIT_TRACK_RECORD_DTYPE is _lib.FIT_TRACK_RECORD_DTYPE
    assert "PARITY UNPINNED" in text[text.index("carrying each camera's fitted pose"):]


def test_layouts_match_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [int(v) for v in consts]
    from depthhead_amd import fit
    assert consts == [fit.FIT_TRACK_NONE, fit.FIT_TRACK_FITTED, fit.FIT_TRACK_CARRIED, fit.FIT_TRACK_REJECTED, fit.FIT_TRACK_ABSENT,
                      fit.FIT_TRACK_BAD_STATUS, fit.FIT_TRACK_BAD_POINTS, fit.FIT_TRACK_BAD_RMS, fit.FIT_TRACK_BAD_JUMP,
                      fit.FIT_TRACK_MOTION, _lib.FIT_TRACK_ANGLES] == [0, 1, 2, 3, 4, 0x100, 0x200, 0x400, 0x800, 1, 120]
    for name, dt, size in (("dh_fit_track_state", _lib.FIT_TRACK_STATE_DTYPE, 76), ("dh_fit_track_record", _lib.FIT_TRACK_RECORD_DTYPE, 104)):
        assert c[(name, "size")] == dt.itemsize == size
        for f in dt.names:
            assert c[(name, f)] == dt.fields[f][1], (name, f)
        # no padding: the fields fill the record
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == size
    assert c[("dh_fit_track_params", "size")] == C.sizeof(_lib.FitTrackParams) == 56
    for f, _ in _lib.FitTrackParams._fields_:
        assert c[("dh_fit_track_params", f)] == getattr(_lib.FitTrackParams, f).offset, f
    # the restatement's records are the same bytes
    import fit_track_ref as ft
    assert ft.STATE.itemsize == 76 and ft.RECORD.itemsize == 104
    for f in ft.RECORD.names:
        assert ft.RECORD.fields[f][1] == _lib.FIT_TRACK_RECORD_DTYPE.fields[f][1]
    for f in ft.STATE.names:
        assert ft.STATE.fields[f][1] == _lib.FIT_TRACK_STATE_DTYPE.fields[f][1]


def default_params(lib):
    p = _lib.FitTrackParams()
    assert lib.dh_fit_track_params_default(C.byref(p)) == 0
    return p


def test_default_params(hip_lib):
    p = default_params(hip_lib)
    assert (p.iterations_tracked, p.keep_points, p.rms_max, p.max_jump, p.conf_num, p.conf_den, p.min_windows, p.max_coast,
            list(p.reserved)) == (6, 30, 5.0, 150.0, 1, 50, 1, 3, [0, 0])
    assert hip_lib.dh_fit_track_params_default(None) == EINVAL and "NULL" in _err(hip_lib)
    import fit_track_ref as ft
    d = ft.params()
    assert (d["iterations_tracked"], d["keep_points"], d["rms_max"], d["max_jump"], d["conf_num"], d["conf_den"], d["min_windows"],
            d["max_coast"]) == (6, 30, 5.0, 150.0, 1, 50, 1, 3)


def test_angle_table_is_within_one_ulp_of_numpy(hip_lib):
    tab = np.full((120, 2), np.nan)
    assert hip_lib.dh_fit_tracker_angles(_lib.vp(tab)) == 0
    a = (np.arange(120) - 60).astype(np.float64) / 60.0 * 3.14159
    for col, want in ((0, np.cos(a)), (1, np.sin(a))):
        assert (np.abs(tab[:, col] - want) <= np.spacing(np.abs(want))).all(), col
    assert tab[60].tolist() == [1.0, 0.0]
    assert hip_lib.dh_fit_tracker_angles(None) == EINVAL and "NULL" in _err(hip_lib)
    again = np.zeros((120, 2))
    hip_lib.dh_fit_tracker_angles(_lib.vp(again))
    assert again.tobytes() == tab.tobytes()


def test_create_refusals(hip_lib):
    lib = hip_lib
    h = C.c_void_p(1234)

    def create(prm=None, flags=0, scale=1.0, out=h, cams=None, model=None):
        return lib.dh_fit_tracker_create(cams, model, C.c_float(scale), C.c_uint32(flags), C.byref(prm) if prm is not None else None,
                                         C.byref(out) if out is not None else None)

    def with_params(**kw):
        p = default_params(lib)
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    assert create(out=None) == EINVAL and "NULL" in _err(lib)
    assert create() == EINVAL and "NULL camera table" in _err(lib) and h.value is None
    assert create(cams=C.c_void_p(8)) == EINVAL and "NULL model" in _err(lib)      # (the table is not looked at before the model is there)
    for flags in (2, 0x80000000, 3):
        assert create(flags=flags) == EINVAL and "unknown flags" in _err(lib)
    for scale in (np.nan, np.inf, -np.inf):
        assert create(scale=scale) == EINVAL and "scale is not finite" in _err(lib)
    assert create(with_params(iterations_tracked=65)) == EINVAL and "iterations_tracked 65 above 64" in _err(lib)
    for field in ("rms_max", "max_jump"):
        for v in (0.0, -1.0, 4096.5, np.nan, np.inf):
            assert create(with_params(**{field: v})) == EINVAL and field in _err(lib), (field, v)
    assert create(with_params(conf_den=0)) == EINVAL and "confidence" in _err(lib)
    assert create(with_params(conf_num=51)) == EINVAL and "confidence 51 / 50" in _err(lib)
    for i in (0, 1):
        assert create(with_params(reserved=i)) == EINVAL and "reserved" in _err(lib)
    # within range: the next refusal (the camera table) answers
    for p in (with_params(iterations_tracked=64), with_params(iterations_tracked=0), with_params(rms_max=4096.0), with_params(conf_num=50),
              with_params(conf_num=0, conf_den=1), with_params(max_coast=0xFFFFFFFF, keep_points=0, min_windows=0)):
        assert create(p) == EINVAL and "NULL camera table" in _err(lib)
    assert create(flags=1) == EINVAL and "NULL camera table" in _err(lib)
    assert h.value is None


def test_refusals_without_a_tracker_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    frames = np.full((1, 8, 8), 800, np.uint16)
    poses, sup = np.zeros(1, _lib.POSE_DTYPE), np.zeros(1, _lib.SUPPORT_DTYPE)
    rec = np.full(104, 0xCD, np.uint8)
    st = np.full(76, 0xAB, np.uint8)
    assert lib.dh_fit_tracker_step_poses(None, vp(frames), 8, 8, None, vp(poses), vp(sup), None, vp(rec)) == EINVAL
    assert "NULL tracker" in _err(lib) and "dh_fit_tracker_step_poses" in _err(lib)
    assert lib.dh_fit_tracker_step_poses_device(None, vp(frames), 8, 8, None, vp(poses), vp(sup), None, vp(rec), None) == EINVAL
    assert "NULL tracker" in _err(lib) and "dh_fit_tracker_step_poses_device" in _err(lib)
    assert lib.dh_fit_tracker_step(None, None, vp(frames), 8, 8, None, 30, None, vp(poses), vp(sup), vp(rec)) == EINVAL
    assert "NULL predictor" in _err(lib)
    assert lib.dh_fit_tracker_step_device(None, None, vp(frames), 8, 8, None, 30, None, vp(poses), vp(sup), vp(rec), None) == EINVAL
    assert "NULL predictor" in _err(lib)
    assert lib.dh_fit_tracker_step(C.c_void_p(8), None, vp(frames), 8, 8, None, 30, None, vp(poses), vp(sup), vp(rec)) == EINVAL
    assert "NULL tracker" in _err(lib)
    assert lib.dh_fit_tracker_step_device(C.c_void_p(8), None, vp(frames), 8, 8, None, 30, None, vp(poses), vp(sup), vp(rec), None) == EINVAL
    assert "NULL tracker" in _err(lib)
    assert lib.dh_fit_tracker_reset(None, -1, None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_fit_tracker_state(None, vp(st)) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_fit_tracker_destroy(None) == 0
    assert (rec == 0xCD).all() and (st == 0xAB).all() and not poses.tobytes().strip(b"\0") and not sup.tobytes().strip(b"\0")
