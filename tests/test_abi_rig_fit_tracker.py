"""The rig fit tracker's entry points without a GPU: exported and declared (and the header's declarations equal _lib.EXPORTS), the
dh_rig_fit_track_params / _state / _record layouts of the Python side equal the C layout (a g++ program prints sizeof and offsetof
from include/depthhead_hip.h), the defaults, and every refusal that can be reached without a device answers DH_EINVAL with a
message and leaves its outputs untouched.  The tables and a model need a device, so a tracker cannot exist here: creation's
parameter refusals are decided before the tables and the model are looked at, and the refusals that need a tracker are in
tests/test_gpu_rig_fit_tracker.py."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_rig_fit_track_params_default", "dh_rig_fit_tracker_create", "dh_rig_fit_tracker_destroy", "dh_rig_fit_tracker_reset",
       "dh_rig_fit_tracker_state", "dh_rig_fit_tracker_step_persons", "dh_rig_fit_tracker_step_persons_device", "dh_rig_fit_tracker_step",
       "dh_rig_fit_tracker_step_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_rig_fit_track_params size %zu\n", sizeof(dh_rig_fit_track_params));
    F(dh_rig_fit_track_params, iterations_tracked); F(dh_rig_fit_track_params, keep_points); F(dh_rig_fit_track_params, rms_max);
    F(dh_rig_fit_track_params, max_jump); F(dh_rig_fit_track_params, max_coast); F(dh_rig_fit_track_params, max_misses);
    F(dh_rig_fit_track_params, reserved);
    printf("dh_rig_fit_state size %zu\n", sizeof(dh_rig_fit_state));
    F(dh_rig_fit_state, id); F(dh_rig_fit_state, R); F(dh_rig_fit_state, t); F(dh_rig_fit_state, t_prev); F(dh_rig_fit_state, views_used);
    F(dh_rig_fit_state, tracked); F(dh_rig_fit_state, have_prev); F(dh_rig_fit_state, age); F(dh_rig_fit_state, lost);
    printf("dh_rig_fit_record size %zu\n", sizeof(dh_rig_fit_record));
    F(dh_rig_fit_record, instance); F(dh_rig_fit_record, fit); F(dh_rig_fit_record, id); F(dh_rig_fit_record, status);
    F(dh_rig_fit_record, age); F(dh_rig_fit_record, lost); F(dh_rig_fit_record, person); F(dh_rig_fit_record, reserved);
    printf("consts %d %d %d\n", DH_RIG_MAX_TRACKS, DH_RIG_MAX_PERSONS, DH_TRACK_MAX_MISSES);
    return 0;
}
"""


def test_entry_points_are_exported_and_the_header_equals_the_export_list(hip_lib):
    text = abi_kit.header()
    abi_kit.assert_exported(hip_lib, NEW)
    abi_kit.assert_header_equals_exports(NEW)
    import depthhead_amd
    from depthhead_amd import fit
    assert hasattr(depthhead_amd, "RigFitTracker") and "RigFitTracker" in depthhead_amd.__all__
    for name in ("step", "step_persons", "step_device", "reset", "state"):
        assert callable(getattr(fit.RigFitTracker, name)), name
    assert callable(fit.rig_fit_track_params)
    section = text[text.index("carrying each rig person's fitted world pose across steps"):]
    assert "PARITY UNPINNED" in section[:2000] and "MUST NOT EXCEED" in section


def test_layouts_match_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [int(v) for v in consts]
    assert consts == [_lib.RIG_MAX_TRACKS, _lib.RIG_MAX_PERSONS, _lib.TRACK_MAX_MISSES] == [16, 16, 3]
    for name, dt, size in (("dh_rig_fit_state", _lib.RIG_FIT_STATE_DTYPE, 88), ("dh_rig_fit_record", _lib.RIG_FIT_RECORD_DTYPE, 128)):
        assert c[(name, "size")] == dt.itemsize == size
        for f in dt.names:
            assert c[(name, f)] == dt.fields[f][1], (name, f)
        # no padding: the fields fill the record
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == size
    assert c[("dh_rig_fit_track_params", "size")] == C.sizeof(_lib.RigFitTrackParams) == 48
    for f, _ in _lib.RigFitTrackParams._fields_:
        assert c[("dh_rig_fit_track_params", f)] == getattr(_lib.RigFitTrackParams, f).offset, f
    # the restatement's records are the same bytes
    import rig_fit_track_ref as rf
    for mine, theirs in ((rf.STATE, _lib.RIG_FIT_STATE_DTYPE), (rf.RECORD, _lib.RIG_FIT_RECORD_DTYPE)):
        assert mine.itemsize == theirs.itemsize and mine.names == theirs.names
        for f in mine.names:
            assert mine.fields[f][1] == theirs.fields[f][1]


def default_params(lib):
    p = _lib.RigFitTrackParams()
    assert lib.dh_rig_fit_track_params_default(C.byref(p)) == 0
    return p


def test_default_params(hip_lib):
    p = default_params(hip_lib)
    assert (p.iterations_tracked, p.keep_points, p.rms_max, p.max_jump, p.max_coast, p.max_misses, list(p.reserved)) == \
        (6, 30, 5.0, 150.0, 3, _lib.TRACK_MAX_MISSES, [0, 0])
    assert hip_lib.dh_rig_fit_track_params_default(None) == EINVAL and "NULL" in _err(hip_lib)
    import rig_fit_track_ref as rf
    d = rf.params()
    assert (d["iterations_tracked"], d["keep_points"], d["rms_max"], d["max_jump"], d["max_coast"], d["max_misses"]) == (6, 30, 5.0, 150.0, 3, 3)
    from depthhead_amd import fit
    q = fit.rig_fit_track_params(max_coast=5, max_misses=6, rms_max=3.0)
    assert (q.max_coast, q.max_misses, q.rms_max, q.iterations_tracked) == (5, 6, 3.0, 6)


def test_create_refusals(hip_lib):
    lib = hip_lib
    h = C.c_void_p(1234)

    def create(prm=None, flags=0, scale=1.0, out=h, rig=None, views=None, model=None):
        return lib.dh_rig_fit_tracker_create(rig, views, model, C.c_float(scale), C.c_uint32(flags), C.byref(prm) if prm is not None else None,
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
    assert create() == EINVAL and "NULL rig table" in _err(lib) and h.value is None
    # (no table is looked at before all three handles are there)
    assert create(rig=C.c_void_p(8)) == EINVAL and "NULL view table" in _err(lib)
    assert create(rig=C.c_void_p(8), views=C.c_void_p(8)) == EINVAL and "NULL model" in _err(lib)
    for flags in (2, 0x80000000, 3):
        assert create(flags=flags) == EINVAL and "unknown flags" in _err(lib)
    for scale in (np.nan, np.inf, -np.inf):
        assert create(scale=scale) == EINVAL and "scale is not finite" in _err(lib)
    assert create(with_params(iterations_tracked=65)) == EINVAL and "iterations_tracked 65 above 64" in _err(lib)
    for field in ("rms_max", "max_jump"):
        for v in (0.0, -1.0, 4096.5, np.nan, np.inf):
            assert create(with_params(**{field: v})) == EINVAL and field in _err(lib), (field, v)
    assert create(with_params(max_coast=4)) == EINVAL and "max_coast 4 above the max_misses 3" in _err(lib)
    assert create(with_params(max_coast=1, max_misses=0)) == EINVAL and "max_coast 1 above the max_misses 0" in _err(lib)
    for i in (0, 1):
        assert create(with_params(reserved=i)) == EINVAL and "reserved" in _err(lib)
    # within range: the next refusal (the rig table) answers
    for p in (with_params(iterations_tracked=64), with_params(iterations_tracked=0), with_params(rms_max=4096.0), with_params(max_coast=0, max_misses=0),
              with_params(max_coast=0xFFFFFFFF, max_misses=0xFFFFFFFF, keep_points=0), with_params(max_coast=3, max_misses=3)):
        assert create(p) == EINVAL and "NULL rig table" in _err(lib)
    assert create(flags=1) == EINVAL and "NULL rig table" in _err(lib)
    assert h.value is None


def test_refusals_without_a_tracker_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    frames = np.full((1, 8, 8), 800, np.uint16)
    n_heads, heads = np.zeros(1, np.uint32), np.zeros((1, 2), _lib.HEAD_DTYPE)
    n_persons, persons = np.zeros(1, np.uint32), np.zeros((1, 16), _lib.RIG_PERSON_DTYPE)
    ids = np.zeros((1, 2), np.uint32)
    rec = np.full(16 * 128, 0xCD, np.uint8)
    st = np.full(16 * 88, 0xAB, np.uint8)
    core = (vp(frames), 8, 8, None, 2, vp(n_heads), vp(heads), vp(n_persons), vp(persons), None, vp(rec))
    assert lib.dh_rig_fit_tracker_step_persons(None, *core) == EINVAL
    assert "NULL tracker" in _err(lib) and "dh_rig_fit_tracker_step_persons" in _err(lib)
    assert lib.dh_rig_fit_tracker_step_persons_device(None, *core, None) == EINVAL
    assert "NULL tracker" in _err(lib) and "dh_rig_fit_tracker_step_persons_device" in _err(lib)
    whole = (vp(frames), 8, 8, None, None, vp(n_heads), vp(heads), vp(ids), vp(n_persons), vp(persons), None, vp(rec))
    assert lib.dh_rig_fit_tracker_step(None, None, None, *whole) == EINVAL and "NULL predictor" in _err(lib)
    assert lib.dh_rig_fit_tracker_step_device(None, None, None, *whole, None) == EINVAL and "NULL predictor" in _err(lib)
    # (neither the predictor nor the rig tracker is looked at before the tracker is there)
    assert lib.dh_rig_fit_tracker_step(C.c_void_p(8), None, C.c_void_p(8), *whole) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_fit_tracker_step_device(C.c_void_p(8), None, C.c_void_p(8), *whole, None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_fit_tracker_reset(None, -1, None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_fit_tracker_state(None, vp(st)) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_fit_tracker_destroy(None) == 0
    assert (rec == 0xCD).all() and (st == 0xAB).all()
    for a in (n_heads, heads, n_persons, persons, ids):
        assert not a.tobytes().strip(b"\0")
