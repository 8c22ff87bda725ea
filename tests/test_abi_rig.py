"""The rig entry points without a GPU: exported and declared, the dh_rig_person / dh_rig_track / dh_rig_track_params layouts of
the Python dtypes equal the C layout (a g++ program prints sizeof and offsetof from include/depthhead_hip.h), and the refusals
that need no device answer DH_EINVAL with a message."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_rig_create", "dh_rig_destroy", "dh_rig_tracker_create", "dh_rig_tracker_destroy", "dh_rig_tracker_reset",
       "dh_rig_tracker_step", "dh_rig_tracker_step_device", "dh_rig_tracker_state", "dh_rig_tracker_capture"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_rig_person size %zu\n", sizeof(dh_rig_person));
    printf("dh_rig_person align %zu\n", alignof(dh_rig_person));
    F(dh_rig_person, views); F(dh_rig_person, mass); F(dh_rig_person, cell); F(dh_rig_person, n_views); F(dh_rig_person, world);
    F(dh_rig_person, id); F(dh_rig_person, best_cam); F(dh_rig_person, best_head);
    printf("dh_rig_track size %zu\n", sizeof(dh_rig_track));
    printf("dh_rig_track align %zu\n", alignof(dh_rig_track));
    F(dh_rig_track, id); F(dh_rig_track, age); F(dh_rig_track, hits); F(dh_rig_track, misses); F(dh_rig_track, person);
    printf("dh_rig_track_params size %zu\n", sizeof(dh_rig_track_params));
    F(dh_rig_track_params, max_heads); F(dh_rig_track_params, radius); F(dh_rig_track_params, fuse_gate);
    F(dh_rig_track_params, gate); F(dh_rig_track_params, max_misses);
    printf("consts %d %d %d %d\n", DH_RIG_MAX_CAMERAS, DH_RIG_MAX_PERSONS, DH_RIG_MAX_TRACKS, DH_RIG_FUSE_GATE);
    return 0;
}
"""


def test_rig_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    from depthhead_amd import tracking
    for m in ("step", "step_device", "capture", "reset", "state", "close", "__enter__", "__exit__"):
        assert hasattr(tracking.RigTracker, m), m
    assert hasattr(tracking.Rig, "close") and callable(tracking.world_rotation)


def test_header_declares_every_rig_export():
    abi_kit.assert_header_equals_exports(NEW)


def test_layouts_match_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [int(v) for v in consts]
    assert consts == [_lib.RIG_MAX_CAMERAS, _lib.RIG_MAX_PERSONS, _lib.RIG_MAX_TRACKS, _lib.RIG_FUSE_GATE] == [64, 16, 16, 100]
    for name, dt in (("dh_rig_person", _lib.RIG_PERSON_DTYPE), ("dh_rig_track", _lib.RIG_TRACK_DTYPE)):
        assert c[(name, "size")] == dt.itemsize and c[(name, "align")] == 8, name
        for f in dt.names:
            assert c[(name, f)] == dt.fields[f][1], (name, f)
        # no padding: the fields tile the record
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == dt.itemsize, name
    assert c[("dh_rig_track_params", "size")] == C.sizeof(_lib.RigTrackParams) == 20
    for f, _ in _lib.RigTrackParams._fields_:
        assert c[("dh_rig_track_params", f)] == getattr(_lib.RigTrackParams, f).offset, f


def _params(max_heads=4, radius=30, fuse_gate=100, gate=100, max_misses=3):
    return _lib.RigTrackParams(max_heads, radius & 0xFFFFFFFF, fuse_gate & 0xFFFFFFFF, gate & 0xFFFFFFFF, max_misses)


def test_create_refusals(hip_lib):
    lib = hip_lib
    h = C.c_void_p(1234)
    R = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    t = np.zeros((2, 3), dtype=np.float32)
    rb = np.array([0, 2], dtype=np.int32)
    vp = _lib.vp
    assert lib.dh_rig_create(None, vp(R), vp(t), vp(rb), 1, C.byref(h)) == EINVAL
    assert "NULL" in _err(lib) and h.value is None       # *out cleared on failure
    assert lib.dh_rig_create(None, vp(R), vp(t), vp(rb), 1, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_rig_destroy(None) == 0
    h = C.c_void_p(1234)
    assert lib.dh_rig_tracker_create(None, C.byref(_params()), C.byref(h)) == EINVAL
    assert "NULL rig table" in _err(lib) and h.value is None
    assert lib.dh_rig_tracker_create(None, None, C.byref(h)) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_rig_tracker_create(None, C.byref(_params()), None) == EINVAL
    for mh in (0, 5, -1):
        assert lib.dh_rig_tracker_create(None, C.byref(_params(max_heads=mh)), C.byref(h)) == EINVAL
        assert "max_heads" in _err(lib), mh
    for r in (-1, 1 << 31):
        for field in ("radius", "fuse_gate", "gate"):
            assert lib.dh_rig_tracker_create(None, C.byref(_params(**{field: r})), C.byref(h)) == EINVAL
            assert field in _err(lib), (field, r)
    big = (1 << 31) - 1
    assert lib.dh_rig_tracker_create(None, C.byref(_params(1, big, big, big, 0xFFFFFFFF)), C.byref(h)) == EINVAL
    assert "NULL rig table" in _err(lib)
    assert lib.dh_rig_tracker_destroy(None) == 0


def test_step_and_state_refusals(hip_lib):
    lib = hip_lib
    buf = np.zeros(64, dtype=np.uint8)
    b = buf.ctypes.data_as(C.c_void_p)
    assert lib.dh_rig_tracker_reset(None, -1, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_rig_tracker_state(None, None, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_rig_tracker_step(None, None, b, 64, 64, None, b, b, b, b, b, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_rig_tracker_step_device(None, None, b, 64, 64, None, b, b, b, b, b, None, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_rig_tracker_capture(None, None, b, 64, 64, None, b, b, b, b, b, None) == EINVAL and "NULL" in _err(lib)


def test_world_rotation_takes_a_pose_rotation_in_radians():
    """The unit is dh_pose.rotation's (radians, multiples of 3.14159 / 60) and the convention the reference viewer's
    (utils/src/headwin.rs:82-84, 115, 150-169, 285): rotx(-rot[2]) roty(-rot[1]) rotz(rot[0]) in a frame with y negated."""
    from depthhead_amd.tracking import world_rotation
    I, q = np.eye(3), np.pi / 2
    assert np.allclose(world_rotation(I, (0, 0, 0)), I)
    # quarter turns, worked by hand from the viewer's matrices: rot[0] turns about z, and the y flip reverses its sense;
    # rot[1] about y keeps its sense; rot[2] about x is negated by the viewer and again by the flip
    assert np.allclose(world_rotation(I, (q, 0, 0)), [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], atol=1e-12)
    assert np.allclose(world_rotation(I, (0, q, 0)), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-12)
    assert np.allclose(world_rotation(I, (0, 0, q)), [[1, 0, 0], [0, 0, -1], [0, 1, 0]], atol=1e-12)
    # the order: rot[0] acts on the model first, rot[2] last
    assert np.allclose(world_rotation(I, (q, 0, q)), np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]]) @ [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], atol=1e-12)
    # a rotation as a dh_pose record holds it: one step of the rotation grid is 3.14159 / 60 rad = 3 degrees, not 0.05 degrees
    pose = np.zeros((), dtype=_lib.POSE_DTYPE)
    pose["rotation"] = (3.14159 / 60, 0.0, -2 * 3.14159 / 60)
    m = world_rotation(I, pose["rotation"])
    assert np.allclose(m @ m.T, I, atol=1e-12) and np.isclose(np.linalg.det(m), 1.0)
    assert np.isclose(np.degrees(np.arccos(m[2, 2])), 6.0, atol=1e-3)        # the model's z axis is tilted by rot[2] alone
    assert np.isclose(np.degrees(np.arctan2(m[0, 1], m[0, 0])), 3.0, atol=1e-3)         # and its x axis turned by rot[0] alone
    # the camera's extrinsic rotation comes last
    Rz90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    assert np.allclose(world_rotation(Rz90, (q, 0, 0)), I, atol=1e-12)
