"""The rig subject fit tracker's entry points without a GPU: exported and declared, the dh_rig_subject_state /
_record layouts of the Python side and of the restatement equal the C layout (a g++ program prints sizeof and offsetof from
include/depthhead_hip.h: 104 and 184 bytes, no padding), the defaults creation selects, and every refusal that can be reached
without a device, in the header's order, answers DH_EINVAL with a message and leaves its outputs untouched.  A rig table, a view
table, a set and a model need a device, so a tracker cannot exist here: the refusals past the NULL handles (the view table's camera
table, the ident params, the reserved words of the dh_subject_track_params, devices, point counts, extents, terms, pairs) and those
that need a tracker, bind's among them, are in tests/test_gpu_rig_subject_tracker.py."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_rig_subject_fit_tracker_create", "dh_rig_subject_fit_tracker_destroy", "dh_rig_subject_fit_tracker_reset",
       "dh_rig_subject_fit_tracker_state", "dh_rig_subject_fit_tracker_info", "dh_rig_subject_fit_tracker_set_enrolled",
       "dh_rig_subject_fit_tracker_bind", "dh_rig_subject_fit_tracker_step_persons", "dh_rig_subject_fit_tracker_step_persons_device",
       "dh_rig_subject_fit_tracker_step", "dh_rig_subject_fit_tracker_step_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_rig_subject_state size %zu\n", sizeof(dh_rig_subject_state));
    F(dh_rig_subject_state, fit); F(dh_rig_subject_state, subject); F(dh_rig_subject_state, wait); F(dh_rig_subject_state, tries);
    F(dh_rig_subject_state, bound_age);
    printf("dh_rig_subject_record size %zu\n", sizeof(dh_rig_subject_record));
    F(dh_rig_subject_record, track); F(dh_rig_subject_record, ident); F(dh_rig_subject_record, subject); F(dh_rig_subject_record, model);
    F(dh_rig_subject_record, identified); F(dh_rig_subject_record, tries);
    printf("dh_rig_fit_state size %zu\n", sizeof(dh_rig_fit_state));
    printf("dh_rig_fit_record size %zu\n", sizeof(dh_rig_fit_record));
    return 0;
}
"""


def test_rig_subject_tracker_entry_points_are_exported_and_declared(hip_lib):
    text = abi_kit.header()
    abi_kit.assert_exported(hip_lib, NEW)
    abi_kit.assert_header_equals_exports(NEW)
    import depthhead_amd
    from depthhead_amd import fit
    assert hasattr(depthhead_amd, "RigSubjectFitTracker") and "RigSubjectFitTracker" in depthhead_amd.__all__
    for name in ("step", "step_persons", "step_device", "reset", "state", "info", "bind", "set_enrolled"):
        assert callable(getattr(fit.RigSubjectFitTracker, name)), name
    section = text[text.index("following each rig person with its own subject's model"):]
    assert "PARITY UNPINNED" in section[:section.index("typedef struct dh_rig_subject_state")]
    assert text.index("following each tracked head with its own subject's model") < text.index("following each rig person with its own subject's model")
    from depthhead_amd import build
    assert "k_rig_subject_track.hip" in build.SOURCES


def test_layouts_match_the_header(tmp_path):
    c, _ = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    import rig_subject_track_ref as rs
    for name, dt, ref, size in (("dh_rig_subject_state", _lib.RIG_SUBJECT_STATE_DTYPE, rs.STATE, 104),
                                ("dh_rig_subject_record", _lib.RIG_SUBJECT_RECORD_DTYPE, rs.RECORD, 184)):
        assert c[(name, "size")] == dt.itemsize == ref.itemsize == size
        assert dt.names == ref.names
        for f in dt.names:
            assert c[(name, f)] == dt.fields[f][1] == ref.fields[f][1], (name, f)
        # no padding: the fields fill the record
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == size
    assert c[("dh_rig_subject_state", "fit")] == 0 and c[("dh_rig_subject_state", "subject")] == c[("dh_rig_fit_state", "size")] == 88
    assert c[("dh_rig_subject_record", "track")] == 0 and c[("dh_rig_subject_record", "ident")] == c[("dh_rig_fit_record", "size")] == 128
    assert _lib.RIG_SUBJECT_STATE_DTYPE.fields["fit"][0] == _lib.RIG_FIT_STATE_DTYPE
    assert _lib.RIG_SUBJECT_RECORD_DTYPE.fields["track"][0] == _lib.RIG_FIT_RECORD_DTYPE
    assert _lib.RIG_SUBJECT_RECORD_DTYPE.fields["ident"][0] == _lib.IDENT_RECORD_DTYPE
    # a free entry: zeros with subject = DH_IDENT_UNKNOWN
    free = rs.initial(1)[0]
    assert free["subject"] == _lib.IDENT_UNKNOWN and not free["fit"].tobytes().strip(b"\0") and (free["wait"], free["tries"], free["bound_age"]) == (0, 0, 0)


def test_the_defaults_creation_selects(hip_lib):
    """NULL params select section 22's, section 28's and section 29's defaults; the restatement's are the same."""
    import ident_views_ref as ivr
    import rig_fit_track_ref as rf
    import rig_subject_track_ref as rs
    t = _lib.RigFitTrackParams()
    assert hip_lib.dh_rig_fit_track_params_default(C.byref(t)) == 0
    assert {f: getattr(t, f) for f in rf.params()} == rf.params()
    i = _lib.IdentParams()
    assert hip_lib.dh_fit_ident_views_params_default(C.byref(i)) == 0
    want = ivr.params()
    assert (i.iterations, i.min_points, i.gate, i.lam, i.max_rms, i.min_ratio) == tuple(want[k] for k in ("iterations", "min_points", "gate", "lambda", "max_rms", "min_ratio"))
    assert i.max_rms == _lib.IDENT_VIEWS_DEFAULT_MAX_RMS == 2.58
    p = _lib.SubjectTrackParams()
    assert hip_lib.dh_subject_track_params_default(C.byref(p)) == 0
    assert rs.params() == {"retry": p.retry, "max_tries": p.max_tries} == {"retry": 4, "max_tries": 4}


def test_create_refusals_in_the_headers_order(hip_lib):
    """Every refusal before the handles are looked at, each with all LATER faults present too: the earlier one answers."""
    lib = hip_lib
    h = C.c_void_p(1234)

    def create(prm=None, flags=0, scale=1.0, out=h, rig=None, views=None, st=None, model=None, ident=None, sub=None):
        return lib.dh_rig_subject_fit_tracker_create(rig, views, st, model, C.c_float(scale), C.c_uint32(flags), _lib.ref(prm), _lib.ref(ident),
                                                     _lib.ref(sub), None, C.byref(out) if out is not None else None)

    def with_params(**kw):
        p = _lib.RigFitTrackParams()
        assert lib.dh_rig_fit_track_params_default(C.byref(p)) == 0
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    bad_ident = _lib.IdentParams()
    assert lib.dh_fit_ident_views_params_default(C.byref(bad_ident)) == 0
    bad_ident.iterations = 65
    bad_sub = _lib.SubjectTrackParams()
    bad_sub.reserved[1] = 1
    later = dict(ident=bad_ident, sub=bad_sub)
    assert create(out=None) == EINVAL and "NULL" in _err(lib)
    # the faults in the header's order; fault i is tried with every fault after it present too, and the NULL handles and bad params after them
    faults = [("flags", "unknown flags"), ("scale", "scale is not finite"), ("iterations_tracked", "iterations_tracked 65 above 64"),
              ("rms_max", "rms_max"), ("max_jump", "max_jump"), ("max_coast", "max_coast 4 above the max_misses 3"),
              ("reserved", "reserved word of the params")]
    bad = dict(iterations_tracked=dict(iterations_tracked=65), rms_max=dict(rms_max=0.0), max_jump=dict(max_jump=np.nan),
               max_coast=dict(max_coast=4, max_misses=3), reserved=dict(reserved=1))
    for i, (_, what) in enumerate(faults):
        fields = {}
        for name, _ in faults[max(i, 2):]:
            fields.update(bad[name])
        rc = create(prm=with_params(**fields), flags=2 if i == 0 else 0, scale=np.nan if i <= 1 else 1.0, **later)
        assert rc == EINVAL and what in _err(lib) and "dh_rig_subject_fit_tracker_create" in _err(lib), (what, _err(lib))
        assert h.value is None
    assert create(**later) == EINVAL and "NULL rig table" in _err(lib)
    assert create(rig=C.c_void_p(8), **later) == EINVAL and "NULL view table" in _err(lib)
    assert create(rig=C.c_void_p(8), views=C.c_void_p(8), **later) == EINVAL and "NULL subject set" in _err(lib)
    assert create(rig=C.c_void_p(8), views=C.c_void_p(8), st=C.c_void_p(8), **later) == EINVAL and "NULL model" in _err(lib)   # (no handle is read before all four are there)
    for scale in (np.inf, -np.inf):
        assert create(scale=scale) == EINVAL and "scale is not finite" in _err(lib)
    for flags in (0x80000000, 3):
        assert create(flags=flags) == EINVAL and "unknown flags" in _err(lib)
    # within range: the next refusal (the rig table) answers
    for p in (with_params(iterations_tracked=64), with_params(rms_max=4096.0), with_params(max_coast=3, max_misses=3)):
        assert create(p) == EINVAL and "NULL rig table" in _err(lib)
    assert create(flags=1) == EINVAL and "NULL rig table" in _err(lib) and h.value is None


def test_refusals_without_a_tracker_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    frames = np.full((1, 8, 8), 800, np.uint16)
    n_heads, heads = np.zeros(1, np.uint32), np.zeros((1, 1), _lib.HEAD_DTYPE)
    n_persons, persons = np.zeros(1, np.uint32), np.zeros((1, 16), _lib.RIG_PERSON_DTYPE)
    ids, tracks = np.zeros((1, 1), np.uint32), np.zeros((1, 16), _lib.RIG_TRACK_DTYPE)
    rec = np.full(16 * 184, 0xCD, np.uint8)
    st = np.full(16 * 104, 0xAB, np.uint8)
    n, s, g = C.c_int(-7), C.c_uint32(77), C.c_uint32(77)
    core = (vp(frames), 8, 8, None, 1, vp(n_heads), vp(heads), vp(n_persons), vp(persons), None, vp(rec))
    assert lib.dh_rig_subject_fit_tracker_step_persons(None, *core) == EINVAL
    assert "NULL tracker" in _err(lib) and "dh_rig_subject_fit_tracker_step_persons" in _err(lib)
    assert lib.dh_rig_subject_fit_tracker_step_persons_device(None, *core, None) == EINVAL
    assert "NULL tracker" in _err(lib) and "dh_rig_subject_fit_tracker_step_persons_device" in _err(lib)
    whole = (vp(frames), 8, 8, None, None, vp(n_heads), vp(heads), vp(ids), vp(n_persons), vp(persons), vp(tracks), vp(rec))
    for name, extra in (("dh_rig_subject_fit_tracker_step", ()), ("dh_rig_subject_fit_tracker_step_device", (None,))):
        fn = getattr(lib, name)
        assert fn(None, None, None, *whole, *extra) == EINVAL and "NULL predictor" in _err(lib) and name in _err(lib)
        assert fn(C.c_void_p(8), None, None, *whole, *extra) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_subject_fit_tracker_reset(None, -1, None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_subject_fit_tracker_state(None, vp(st)) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_subject_fit_tracker_info(None, C.byref(n), C.byref(s), C.byref(g)) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_subject_fit_tracker_bind(None, 0, C.c_uint32(1), C.c_uint32(0), None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_subject_fit_tracker_set_enrolled(None, None, None) == EINVAL and "NULL tracker" in _err(lib)
    assert lib.dh_rig_subject_fit_tracker_destroy(None) == 0
    assert (rec == 0xCD).all() and (st == 0xAB).all()
    for a in (heads, persons, ids, tracks, n_heads, n_persons):
        assert not a.tobytes().strip(b"\0")
    assert (n.value, s.value, g.value) == (-7, 77, 77)
