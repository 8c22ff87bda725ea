"""The multi-head tracker entry points without a GPU: exported and declared, the dh_head_track / dh_multi_track_params layouts
of the Python dtypes equal the C layout (a g++ program prints sizeof and offsetof from include/depthhead_hip.h), and the
refusals that need no device answer DH_EINVAL with a message."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_multi_tracker_create", "dh_multi_tracker_destroy", "dh_multi_tracker_reset", "dh_multi_tracker_step",
       "dh_multi_tracker_step_device", "dh_multi_tracker_state", "dh_multi_tracker_capture"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_head_track size %zu\n", sizeof(dh_head_track));
    F(dh_head_track, id); F(dh_head_track, age); F(dh_head_track, hits); F(dh_head_track, misses); F(dh_head_track, head);
    printf("dh_head size %zu\n", sizeof(dh_head));
    F(dh_head, pose); F(dh_head, support);
    printf("dh_multi_track_params size %zu\n", sizeof(dh_multi_track_params));
    F(dh_multi_track_params, max_heads); F(dh_multi_track_params, radius); F(dh_multi_track_params, gate);
    F(dh_multi_track_params, max_misses);
    printf("consts %d %d %d %d\n", DH_MAX_TRACKS, DH_TRACK_GATE, DH_TRACK_MAX_MISSES, DH_MAX_HEADS);
    return 0;
}
"""


def test_multi_tracker_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    from depthhead_amd import tracking
    for m in ("step", "step_device", "capture", "reset", "state", "close", "__enter__", "__exit__"):
        assert hasattr(tracking.MultiHeadTracker, m), m


def test_layouts_match_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [int(v) for v in consts]
    assert consts == [_lib.MAX_TRACKS, _lib.TRACK_GATE, _lib.TRACK_MAX_MISSES, _lib.MAX_HEADS]
    for name, dt in (("dh_head_track", _lib.TRACK_DTYPE), ("dh_head", _lib.HEAD_DTYPE)):
        assert c[(name, "size")] == dt.itemsize, name
        for f in dt.names:
            assert c[(name, f)] == dt.fields[f][1], (name, f)
    assert c[("dh_multi_track_params", "size")] == C.sizeof(_lib.MultiTrackParams)
    for f, _ in _lib.MultiTrackParams._fields_:
        assert c[("dh_multi_track_params", f)] == getattr(_lib.MultiTrackParams, f).offset, f
    assert _lib.TRACK_DTYPE.itemsize == 96 and _lib.TRACK_DTYPE.fields["head"][1] == 16


def _params(max_heads=4, radius=30, gate=100, max_misses=3):
    return _lib.MultiTrackParams(max_heads, radius & 0xFFFFFFFF, gate & 0xFFFFFFFF, max_misses)


def test_create_refusals(hip_lib):
    lib = hip_lib
    h = C.c_void_p(1234)
    assert lib.dh_multi_tracker_create(None, C.byref(_params()), C.byref(h)) == EINVAL
    assert "NULL" in _err(lib) and h.value is None       # *out cleared on failure
    assert lib.dh_multi_tracker_create(None, None, C.byref(h)) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_multi_tracker_create(None, C.byref(_params()), None) == EINVAL
    for mh in (0, 5, -1):
        assert lib.dh_multi_tracker_create(None, C.byref(_params(max_heads=mh)), C.byref(h)) == EINVAL
        assert "max_heads" in _err(lib), mh
    for r in (-1, 1 << 31):
        assert lib.dh_multi_tracker_create(None, C.byref(_params(radius=r)), C.byref(h)) == EINVAL
        assert "radius" in _err(lib), r
        assert lib.dh_multi_tracker_create(None, C.byref(_params(gate=r)), C.byref(h)) == EINVAL
        assert "gate" in _err(lib), r
    # the largest values are accepted as far as the parameters go (then the NULL table is refused)
    assert lib.dh_multi_tracker_create(None, C.byref(_params(1, (1 << 31) - 1, (1 << 31) - 1, 0xFFFFFFFF)), C.byref(h)) == EINVAL
    assert "NULL camera table" in _err(lib)
    assert lib.dh_multi_tracker_destroy(None) == 0


def test_step_and_state_refusals(hip_lib):
    lib = hip_lib
    buf = np.zeros(64, dtype=np.uint8)
    b = buf.ctypes.data_as(C.c_void_p)
    assert lib.dh_multi_tracker_reset(None, -1, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_multi_tracker_state(None, None, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_multi_tracker_step(None, None, b, 64, 64, None, b, b, b, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_multi_tracker_step_device(None, None, b, 64, 64, None, b, b, b, None, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_multi_tracker_capture(None, None, b, 64, 64, None, b, b, b, None) == EINVAL and "NULL" in _err(lib)
