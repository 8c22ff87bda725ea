"""The camera-table and tracker entry points without a GPU: exported, declared, and their argument checks that need no
device (NULL pointers, n <= 0) answer DH_EINVAL with a message."""
import ctypes as C

import numpy as np

import abi_kit

NEW = ["dh_cameras_create", "dh_cameras_destroy", "dh_predict_batch_cameras", "dh_predict_batch_cameras_device",
       "dh_tracker_create", "dh_tracker_destroy", "dh_tracker_reset", "dh_tracker_step", "dh_tracker_step_device",
       "dh_tracker_state", "dh_tracker_capture"]


def test_tracking_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)


def test_cameras_create_argument_checks(hip_lib):
    K = np.tile(np.array([560, 0, 320, 0, 560, 240, 0, 0, 1], dtype=np.float32), (3, 1))
    h = C.c_void_p(1234)
    assert hip_lib.dh_cameras_create(None, 3, 0, C.byref(h)) == -1
    assert "NULL" in hip_lib.dh_last_error().decode()
    assert hip_lib.dh_cameras_create(K.ctypes.data_as(C.c_void_p), 3, 0, None) == -1
    for n in (0, -1):
        h = C.c_void_p(1234)
        assert hip_lib.dh_cameras_create(K.ctypes.data_as(C.c_void_p), n, 0, C.byref(h)) == -1
        assert "at least one camera" in hip_lib.dh_last_error().decode()
        assert h.value is None        # *out cleared on failure
    assert hip_lib.dh_cameras_destroy(None) == 0


def test_tracker_and_camera_batch_null_arguments(hip_lib):
    h = C.c_void_p()
    assert hip_lib.dh_tracker_create(None, C.c_uint32(1), C.byref(h)) == -1
    assert hip_lib.dh_tracker_destroy(None) == 0
    assert hip_lib.dh_tracker_reset(None, -1, None) == -1
    assert hip_lib.dh_tracker_state(None, None, None, None) == -1
    assert hip_lib.dh_tracker_step(None, None, None, 64, 64, None, None) == -1
    assert hip_lib.dh_tracker_step_device(None, None, None, 64, 64, None, None, None) == -1
    assert hip_lib.dh_tracker_capture(None, None, None, 64, 64, None, None) == -1
    assert hip_lib.dh_predict_batch_cameras(None, None, 1, 64, 64, None, None, None, None, None) == -1
    assert hip_lib.dh_predict_batch_cameras_device(None, None, 1, 64, 64, None, None, None, None, None, None) == -1
    assert "NULL" in hip_lib.dh_last_error().decode()
