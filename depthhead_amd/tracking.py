"""Several cameras in one batch, and live head tracking on the device (include/depthhead_hip.h: dh_cameras, dh_tracker).

* `Cameras(intrinsics, device)`: an immutable table of per-camera intrinsic matrices on one GPU.  Frame i of a camera batch
  (`HoughPrediction.predict_batch_cameras`) is seen by camera i.
* `HeadTracker(hp, cameras, w, h, prev_guess, sluggish)`: the reference's live loop (examples/live_prediction.rs:79-101) for
  one frame per camera per step -- each camera's pose becomes that camera's next guess without leaving the device.
* `MultiHeadTracker(hp, cameras, w, h, max_heads, radius, gate, max_misses)`: up to MAX_HEADS heads per camera per step, each
  with an id that lasts across steps, matched on the device (dh_multi_tracker).
* `Rig(cameras, R, t, rig_begin)` and `RigTracker(hp, rig, w, h, ...)`: cameras grouped into rigs that share a world frame;
  each step fuses the heads of a rig's cameras into persons and gives each an id that lasts across steps AND cameras
  (dh_rig_tracker).  `world_rotation` composes a camera's R with a head's rotation on the host.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (HEAD_DTYPE, MAX_HEADS, MAX_TRACKS, POSE_DTYPE, RIG_FUSE_GATE, RIG_MAX_PERSONS, RIG_MAX_TRACKS,
                   RIG_PERSON_DTYPE, RIG_TRACK_DTYPE, SUPPORT_DTYPE, SUPPORT_RADIUS, TRACK_DTYPE, TRACK_GATE, TRACK_MAX_MISSES,
                   MultiTrackParams, RigTrackParams, check, vp)
from .prediction import _radius, _stream

TRACK_PREV_GUESS = 1   # DH_TRACK_PREV_GUESS: live_prediction --prevguess
TRACK_SLUGGISH = 2     # DH_TRACK_SLUGGISH:   live_prediction --sluggish


class Cameras(_lib._Handle):
    """`intrinsics`: [n, 3, 3] (or [n, 9]) f32 row-major matrices, or a list of `IntrinsicMatrix`."""
    _handles = (("_h", "dh_cameras_destroy"),)

    def __init__(self, intrinsics, device: int = 0):
        self._lib = _lib.load()
        mats = [getattr(k, "mat", k) for k in intrinsics] if isinstance(intrinsics, (list, tuple)) else intrinsics
        self.K = np.ascontiguousarray(np.asarray(mats, dtype=np.float32).reshape(-1, 9))
        self.n = int(self.K.shape[0])
        self.device = device
        self._h = C.c_void_p()
        check(self._lib.dh_cameras_create(vp(self.K), C.c_int(self.n), C.c_int(device), C.byref(self._h)))

    def __len__(self) -> int:
        return self.n


class _Tracker(_lib._Handle):
    """What both trackers share: the predictor, the camera table, the frame size and the host step's argument checks."""

    def __init__(self, hp, cameras: Cameras, w: int, h: int):
        self._lib = _lib.load()
        self.hp, self.cameras, self.w, self.h = hp, cameras, int(w), int(h)
        self.n = len(cameras)

    def _frames(self, frames) -> np.ndarray:
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        if frames.shape != (self.n, self.h, self.w):
            raise ValueError(f"frames must be [{self.n}, {self.h}, {self.w}]")
        return frames

    def _present(self, present):
        return None if present is None else np.ascontiguousarray(present, dtype=np.uint8).reshape(self.n)


class HeadTracker(_Tracker):
    """One frame per camera per step; the state (midpoint [n, 3] f32, rotation [n, 3] f64, guess mask [n] u8) stays on the
    device.  Steps of one tracker must be stream-ordered.  The camera table must outlive the tracker."""
    _handles = (("_h", "dh_tracker_destroy"),)

    def __init__(self, hp, cameras: Cameras, w: int, h: int, prev_guess: bool = True, sluggish: bool = False):
        super().__init__(hp, cameras, w, h)
        self.flags = (TRACK_PREV_GUESS if prev_guess else 0) | (TRACK_SLUGGISH if sluggish else 0)
        self._h = C.c_void_p()
        check(self._lib.dh_tracker_create(cameras._h, C.c_uint32(self.flags), C.byref(self._h)))
        hp.reserve(self.n, self.w, self.h)      # after this a device step allocates nothing (capturable)

    def step(self, frames, present=None) -> np.ndarray:
        """Host frames [n_cams, h, w] uint16 -> POSE_DTYPE[n_cams]; cameras with present[c] == 0 keep their state."""
        frames = self._frames(frames)
        pr = self._present(present)
        out = np.zeros(self.n, dtype=POSE_DTYPE)
        check(self._lib.dh_tracker_step(self.hp._ph, self._h, vp(frames), C.c_int(self.w), C.c_int(self.h), vp(pr), vp(out)))
        return out

    def step_device(self, frames_ptr: int, out_ptr: int, present_ptr: int = 0, stream: int = 0) -> None:
        """Device frames [n_cams][h][w] u16, poses [n_cams] dh_pose, present [n_cams] u8 or 0; asynchronous on `stream`."""
        check(self._lib.dh_tracker_step_device(self.hp._ph, self._h, vp(frames_ptr), C.c_int(self.w), C.c_int(self.h),
                                               vp(present_ptr or None), vp(out_ptr), _stream(stream)))

    def step_support(self, frames, present=None, radius: int = SUPPORT_RADIUS) -> tuple[np.ndarray, np.ndarray]:
        """`step` that also reports every camera's vote support (absent cameras included): -> (POSE_DTYPE[n_cams],
        SUPPORT_DTYPE[n_cams]).  The state is updated exactly as by `step`."""
        frames = self._frames(frames)
        pr = self._present(present)
        out = np.zeros(self.n, dtype=POSE_DTYPE)
        sup = np.zeros(self.n, dtype=SUPPORT_DTYPE)
        check(self._lib.dh_tracker_step_support(self.hp._ph, self._h, vp(frames), C.c_int(self.w), C.c_int(self.h), vp(pr),
                                                _radius(radius), vp(out), vp(sup)))
        return out, sup

    def step_support_device(self, frames_ptr: int, out_ptr: int, support_ptr: int, present_ptr: int = 0,
                            radius: int = SUPPORT_RADIUS, stream: int = 0) -> None:
        """Device-resident twin of `step_support`: support records [n_cams] dh_support at `support_ptr`.  Asynchronous."""
        check(self._lib.dh_tracker_step_support_device(self.hp._ph, self._h, vp(frames_ptr), C.c_int(self.w), C.c_int(self.h),
                                                       vp(present_ptr or None), _radius(radius), vp(out_ptr),
                                                       vp(support_ptr), _stream(stream)))

    def capture(self, frames_ptr: int, out_ptr: int, present_ptr: int = 0) -> None:
        """Capture one device step into the predictor's graph slot; every `hp.graph_launch()` is then one step."""
        check(self._lib.dh_tracker_capture(self.hp._ph, self._h, vp(frames_ptr), C.c_int(self.w), C.c_int(self.h),
                                           vp(present_ptr or None), vp(out_ptr)))

    def reset(self, camera: int | None = None, stream: int = 0) -> None:
        """The reference's initial state ([0, 0, 0], no rotation) for one camera or all; stream-ordered."""
        check(self._lib.dh_tracker_reset(self._h, C.c_int(-1 if camera is None else int(camera)), _stream(stream)))

    def state(self) -> dict:
        """Synchronous copy of the state: midp [n, 3] f32, rot [n, 3] f64, mask [n] u8 (bit0 midpoint guess, bit1
        rotation guess) and has_rot [n] bool."""
        midp = np.zeros((self.n, 3), dtype=np.float32)
        rot = np.zeros((self.n, 3), dtype=np.float64)
        flags = np.zeros(self.n, dtype=np.uint8)
        check(self._lib.dh_tracker_state(self._h, vp(midp), vp(rot), vp(flags)))
        return {"midp": midp, "rot": rot, "mask": flags & 3, "has_rot": (flags & 4) != 0}


class MultiHeadTracker(_Tracker):
    """Several heads per camera with identities that last across steps (include/depthhead_hip.h: dh_multi_tracker, DESIGN.md
    section 15).  Each step runs the heads pipeline on one frame per camera and matches its heads to the camera's tracks on the
    device: every head gets a u32 id, 0 for none.  The state (TRACK_DTYPE [n, MAX_TRACKS] and the next id [n]) stays on the
    device.  Steps of one tracker must be stream-ordered.  The camera table must outlive the tracker."""
    _handles = (("_h", "dh_multi_tracker_destroy"),)

    def __init__(self, hp, cameras: Cameras, w: int, h: int, max_heads: int = MAX_HEADS, radius: int = SUPPORT_RADIUS,
                 gate: int = TRACK_GATE, max_misses: int = TRACK_MAX_MISSES):
        super().__init__(hp, cameras, w, h)
        self.max_heads = int(max_heads)
        self.params = MultiTrackParams(self.max_heads, _radius(radius).value, _radius(gate).value,
                                       int(max_misses) & 0xFFFFFFFF)
        self._h = C.c_void_p()
        check(self._lib.dh_multi_tracker_create(cameras._h, C.byref(self.params), C.byref(self._h)))
        hp.reserve(self.n, self.w, self.h)

    def step(self, frames, present=None, tracks: bool = True):
        """Host frames [n_cams, h, w] uint16 -> (n_heads u32 [n_cams], HEAD_DTYPE [n_cams, max_heads], ids u32 [n_cams,
        max_heads], TRACK_DTYPE [n_cams, MAX_TRACKS] after the step, or None with tracks=False).  Cameras with present[c] == 0
        keep their tracks and get ids of zeros."""
        frames = self._frames(frames)
        pr = self._present(present)
        n_heads = np.zeros(self.n, dtype=np.uint32)
        heads = np.zeros((self.n, self.max_heads), dtype=HEAD_DTYPE)
        ids = np.zeros((self.n, self.max_heads), dtype=np.uint32)
        tr = np.zeros((self.n, MAX_TRACKS), dtype=TRACK_DTYPE) if tracks else None
        check(self._lib.dh_multi_tracker_step(self.hp._ph, self._h, vp(frames), C.c_int(self.w), C.c_int(self.h), vp(pr),
                                              vp(n_heads), vp(heads), vp(ids), vp(tr)))
        return n_heads, heads, ids, tr

    def step_device(self, frames_ptr: int, n_heads_ptr: int, heads_ptr: int, ids_ptr: int, tracks_ptr: int = 0,
                    present_ptr: int = 0, stream: int = 0) -> None:
        """Device frames [n_cams][h][w] u16; n_heads [n_cams] u32, heads [n_cams][max_heads] dh_head, ids [n_cams][max_heads]
        u32, tracks [n_cams][MAX_TRACKS] dh_head_track or 0, present [n_cams] u8 or 0.  Asynchronous on `stream`."""
        check(self._lib.dh_multi_tracker_step_device(self.hp._ph, self._h, vp(frames_ptr), C.c_int(self.w), C.c_int(self.h),
                                                     vp(present_ptr or None), vp(n_heads_ptr), vp(heads_ptr), vp(ids_ptr),
                                                     vp(tracks_ptr or None), _stream(stream)))

    def capture(self, frames_ptr: int, n_heads_ptr: int, heads_ptr: int, ids_ptr: int, tracks_ptr: int = 0,
                present_ptr: int = 0) -> None:
        """Capture one device step into the predictor's graph slot; every `hp.graph_launch()` is then one step."""
        check(self._lib.dh_multi_tracker_capture(self.hp._ph, self._h, vp(frames_ptr), C.c_int(self.w), C.c_int(self.h),
                                                 vp(present_ptr or None), vp(n_heads_ptr), vp(heads_ptr), vp(ids_ptr),
                                                 vp(tracks_ptr or None)))

    def reset(self, camera: int | None = None, stream: int = 0) -> None:
        """Every slot of one camera or all free again, next id 1; stream-ordered."""
        check(self._lib.dh_multi_tracker_reset(self._h, C.c_int(-1 if camera is None else int(camera)), _stream(stream)))

    def state(self) -> tuple[np.ndarray, np.ndarray]:
        """Synchronous copy of the state: (TRACK_DTYPE [n, MAX_TRACKS], next id u32 [n])."""
        tr = np.zeros((self.n, MAX_TRACKS), dtype=TRACK_DTYPE)
        nid = np.zeros(self.n, dtype=np.uint32)
        check(self._lib.dh_multi_tracker_state(self._h, vp(tr), vp(nid)))
        return tr, nid


class Rig(_lib._Handle):
    """The extrinsics of every camera of `cameras` and their grouping into rigs (dh_rig).  `R`: [n, 3, 3] (or [n, 9]) f32
    row-major, `t`: [n, 3] f32 in mm -- camera c carries a camera-space point m to the world point R[c] @ m + t[c]; R need not
    be orthonormal.  `rig_begin`: [n_rigs + 1] ascending camera indices from 0 to n, each rig holding 1 .. 64 cameras (default:
    one rig of all cameras).  The camera table must outlive the rig table."""
    _handles = (("_h", "dh_rig_destroy"),)

    def __init__(self, cameras: Cameras, R, t, rig_begin=None):
        self._lib = _lib.load()
        self.cameras, self.n = cameras, len(cameras)
        self.R = np.ascontiguousarray(np.asarray(R, dtype=np.float32).reshape(-1, 9))
        self.t = np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(-1, 3))
        if self.R.shape[0] != self.n or self.t.shape[0] != self.n:
            raise ValueError(f"R must be [{self.n}, 3, 3] and t [{self.n}, 3]")
        self.rig_begin = np.ascontiguousarray([0, self.n] if rig_begin is None else rig_begin, dtype=np.int32).reshape(-1)
        if self.rig_begin.size < 2:
            raise ValueError("rig_begin must hold n_rigs + 1 entries")
        self.n_rigs = int(self.rig_begin.size) - 1
        self._h = C.c_void_p()
        check(self._lib.dh_rig_create(cameras._h, vp(self.R), vp(self.t), vp(self.rig_begin), C.c_int(self.n_rigs),
                                      C.byref(self._h)))

    def __len__(self) -> int:
        return self.n_rigs


class RigTracker(_Tracker):
    """Heads fused across the cameras of each rig into persons with ids that last across steps and cameras (include/
    depthhead_hip.h: dh_rig_tracker).  Each step runs the heads pipeline on one frame per camera and one
    kernel that carries the heads into their rig's world frame, fuses them and matches the persons to the rig's tracks.  The
    state (RIG_TRACK_DTYPE [n_rigs, RIG_MAX_TRACKS] and the next id [n_rigs]) stays on the device.  Steps of one tracker must
    be stream-ordered.  The rig table must outlive the tracker."""
    _handles = (("_h", "dh_rig_tracker_destroy"),)

    def __init__(self, hp, rig: Rig, w: int, h: int, max_heads: int = MAX_HEADS, radius: int = SUPPORT_RADIUS,
                 fuse_gate: int = RIG_FUSE_GATE, gate: int = TRACK_GATE, max_misses: int = TRACK_MAX_MISSES):
        super().__init__(hp, rig.cameras, w, h)
        self.rig, self.n_rigs, self.max_heads = rig, rig.n_rigs, int(max_heads)
        self.params = RigTrackParams(self.max_heads, _radius(radius).value, _radius(fuse_gate).value, _radius(gate).value,
                                     int(max_misses) & 0xFFFFFFFF)
        self._h = C.c_void_p()
        check(self._lib.dh_rig_tracker_create(rig._h, C.byref(self.params), C.byref(self._h)))
        hp.reserve(self.n, self.w, self.h)

    def step(self, frames, present=None, tracks: bool = True):
        """Host frames [n_cams, h, w] uint16 -> (n_heads u32 [n_cams], HEAD_DTYPE [n_cams, max_heads], rig_ids u32 [n_cams,
        max_heads], n_persons u32 [n_rigs], RIG_PERSON_DTYPE [n_rigs, RIG_MAX_PERSONS], RIG_TRACK_DTYPE [n_rigs,
        RIG_MAX_TRACKS] after the step, or None with tracks=False).  Cameras with present[c] == 0 contribute nothing and get ids
        of zeros; a rig without a present camera keeps its state."""
        frames = self._frames(frames)
        pr = self._present(present)
        n_heads = np.zeros(self.n, dtype=np.uint32)
        heads = np.zeros((self.n, self.max_heads), dtype=HEAD_DTYPE)
        ids = np.zeros((self.n, self.max_heads), dtype=np.uint32)
        n_persons = np.zeros(self.n_rigs, dtype=np.uint32)
        persons = np.zeros((self.n_rigs, RIG_MAX_PERSONS), dtype=RIG_PERSON_DTYPE)
        tr = np.zeros((self.n_rigs, RIG_MAX_TRACKS), dtype=RIG_TRACK_DTYPE) if tracks else None
        check(self._lib.dh_rig_tracker_step(self.hp._ph, self._h, vp(frames), C.c_int(self.w), C.c_int(self.h), vp(pr),
                                            vp(n_heads), vp(heads), vp(ids), vp(n_persons), vp(persons), vp(tr)))
        return n_heads, heads, ids, n_persons, persons, tr

    def _device_args(self, frames_ptr, n_heads_ptr, heads_ptr, ids_ptr, n_persons_ptr, persons_ptr, tracks_ptr, present_ptr):
        return (self.hp._ph, self._h, vp(frames_ptr), C.c_int(self.w), C.c_int(self.h), vp(present_ptr or None), vp(n_heads_ptr),
                vp(heads_ptr), vp(ids_ptr), vp(n_persons_ptr), vp(persons_ptr), vp(tracks_ptr or None))

    def step_device(self, frames_ptr: int, n_heads_ptr: int, heads_ptr: int, ids_ptr: int, n_persons_ptr: int, persons_ptr: int,
                    tracks_ptr: int = 0, present_ptr: int = 0, stream: int = 0) -> None:
        """Device frames [n_cams][h][w] u16; n_heads [n_cams] u32, heads [n_cams][max_heads] dh_head, rig_ids
        [n_cams][max_heads] u32, n_persons [n_rigs] u32, persons [n_rigs][RIG_MAX_PERSONS] dh_rig_person, tracks
        [n_rigs][RIG_MAX_TRACKS] dh_rig_track or 0, present [n_cams] u8 or 0.  Asynchronous on `stream`."""
        check(self._lib.dh_rig_tracker_step_device(*self._device_args(frames_ptr, n_heads_ptr, heads_ptr, ids_ptr, n_persons_ptr,
                                                                      persons_ptr, tracks_ptr, present_ptr), _stream(stream)))

    def capture(self, frames_ptr: int, n_heads_ptr: int, heads_ptr: int, ids_ptr: int, n_persons_ptr: int, persons_ptr: int,
                tracks_ptr: int = 0, present_ptr: int = 0) -> None:
        """Capture one device step into the predictor's graph slot; every `hp.graph_launch()` is then one step."""
        check(self._lib.dh_rig_tracker_capture(*self._device_args(frames_ptr, n_heads_ptr, heads_ptr, ids_ptr, n_persons_ptr,
                                                                  persons_ptr, tracks_ptr, present_ptr)))

    def reset(self, rig: int | None = None, stream: int = 0) -> None:
        """Every slot of one rig or all free again, next id 1; stream-ordered."""
        check(self._lib.dh_rig_tracker_reset(self._h, C.c_int(-1 if rig is None else int(rig)), _stream(stream)))

    def state(self) -> tuple[np.ndarray, np.ndarray]:
        """Synchronous copy of the state: (RIG_TRACK_DTYPE [n_rigs, RIG_MAX_TRACKS], next id u32 [n_rigs])."""
        tr = np.zeros((self.n_rigs, RIG_MAX_TRACKS), dtype=RIG_TRACK_DTYPE)
        nid = np.zeros(self.n_rigs, dtype=np.uint32)
        check(self._lib.dh_rig_tracker_state(self._h, vp(tr), vp(nid)))
        return tr, nid


def _euler_matrix(rotation) -> np.ndarray:
    """The rotation matrix of a pose's `rotation` (dh_pose.rotation: three angles in RADIANS, include/depthhead_hip.h) in the
    camera frame of the midpoints (x right, y down, z forward).

    The reference never turns the three angles into a matrix on its prediction path; the one place that does is its viewer,
    which draws the head model turned by rotx(-rot[2]) * roty(-rot[1]) * rotz(rot[0]) in radians (utils/src/headwin.rs:82-84
    with the column-major matrices of :150-169, applied in that order to the vertex at :285; examples/live_prediction.rs:299
    and examples/db_prediction.rs:152 pass it the predicted rotation).  In the usual row convention that is
    V = Rx(-rot[2]) @ Ry(rot[1]) @ Rz(rot[0])  (the viewer's roty is the usual Ry of the opposite angle).  The viewer's frame is
    the camera frame with y negated (it places the model at (x, -y, z), headwin.rs:115), so in the camera frame the matrix is
    F @ V @ F with F = diag(1, -1, 1), which is Rx(rot[2]) @ Ry(rot[1]) @ Rz(-rot[0])."""
    r0, r1, r2 = (float(v) for v in np.asarray(rotation, dtype=np.float64).reshape(3))

    def rx(a):
        return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])

    def ry(a):
        return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])

    def rz(a):
        return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])

    F = np.diag([1.0, -1.0, 1.0])
    return F @ (rx(-r2) @ ry(r1) @ rz(r0)) @ F


def world_rotation(R_cam, rotation) -> np.ndarray:
    """A head's rotation in the world frame: the 3 x 3 matrix R_cam @ E.  `rotation` is a pose's rotation exactly as the library
    reports it -- heads[best_cam][best_head]["pose"]["rotation"] of a person's best view, three angles in radians -- E its
    matrix in that camera's frame by the reference viewer's convention (_euler_matrix), and R_cam that camera's extrinsic
    rotation.  A host helper in numpy f64: it uses sin and cos, which the device and libm do not round alike, and is therefore
    OUTSIDE the library's bit-exact contract -- the rig tracker itself reports rotations in the best view's camera frame only."""
    return np.asarray(R_cam, dtype=np.float64).reshape(3, 3) @ _euler_matrix(rotation)
