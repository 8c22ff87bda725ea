"""Posed head models fitted to depth frames on the GPU: point-to-plane ICP with projective association,
started from a rough pose per head (the forest's), so that position becomes accurate to millimetres and rotation to a few
degrees.  All arithmetic of the fit runs in libdepthhead_hip.so (k_fit.hip); the rule is stated in include/depthhead_hip.h."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import (CALIB_RECORD_DTYPE, CALIB_SKIP, FIT_RECORD_DTYPE, IDENT_RECORD_DTYPE, IDENT_UNKNOWN, FIT_TRACK_ANGLES, FIT_TRACK_RECORD_DTYPE, FIT_TRACK_STATE_DTYPE, FIT_VIEW_TOLERANCE, HEAD_DTYPE,
                   MAX_HEADS, POSE_DTYPE, RIG_FIT_RECORD_DTYPE, RIG_FIT_STATE_DTYPE, RIG_MAX_PERSONS, RIG_MAX_TRACKS, RIG_PERSON_DTYPE,
                   RIG_TRACK_DTYPE, RENDER_INSTANCE_DTYPE, SHAPE_RECORD_DTYPE, SHAPE_SKIP, SUBJECT_STATE_DTYPE, SUPPORT_DTYPE, SUPPORT_RADIUS, SURFACE_RECORD_DTYPE,
                   VIEW_FIT_RECORD_DTYPE,
                   VIEW_INSTANCE_DTYPE, check, vp)
from .render import euler_to_matrix

FIT_OK, FIT_FEW_POINTS, FIT_SINGULAR = 0, 1, 2      # dh_fit_record.status
# dh_fit_track_record.status: the kind in the low byte, the reason bits of a rejected fit above it
FIT_TRACK_NONE, FIT_TRACK_FITTED, FIT_TRACK_CARRIED, FIT_TRACK_REJECTED, FIT_TRACK_ABSENT = 0, 1, 2, 3, 4
FIT_TRACK_BAD_STATUS, FIT_TRACK_BAD_POINTS, FIT_TRACK_BAD_RMS, FIT_TRACK_BAD_JUMP = 0x100, 0x200, 0x400, 0x800
FIT_TRACK_MOTION = 1                                # DH_FIT_TRACK_MOTION
SHAPE_OK, SHAPE_FEW_POINTS, SHAPE_SINGULAR = 0, 1, 2  # dh_shape_record.status
CALIB_OK, CALIB_FEW_POINTS, CALIB_SINGULAR, CALIB_NOT_ORTHONORMAL, CALIB_HELD = 0, 1, 2, 3, 4  # dh_calib_record.status
SUBJECT_CLAMPED, SUBJECT_NONFINITE = 1, 2            # dh_subject_state.flags
SURFACE_OK, SURFACE_FEW_POINTS = 0, 1                # dh_surface_record.status
IDENT_OK, IDENT_SKIPPED, IDENT_NO_CANDIDATE, IDENT_FAR, IDENT_AMBIGUOUS = 0, 1, 2, 3, 4   # dh_ident_record.status


def vertex_normals(verts, tris) -> np.ndarray:
    """Unit vertex normals [nv, 3] f32 of a triangle mesh: the face cross products (v_b - v_a) x (v_c - v_a) added to each of the
    face's three vertices in triangle order, in f64, normalised and rounded to f32 once.  They point outward when the winding
    is counter-clockwise seen from outside (synth.head_mesh's is); nothing is flipped by guessing.  A vertex no triangle with
    area touches gets (0, 0, 0), which dh_fit_model_create refuses."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    n = np.zeros_like(v)
    for a, b, c in t:
        f = np.cross(v[b] - v[a], v[c] - v[a])
        n[a] += f
        n[b] += f
        n[c] += f
    ln = np.sqrt((n * n).sum(axis=1))
    return (n / np.where(ln > 0.0, ln, 1.0)[:, None]).astype(np.float32)


def matrix_to_euler(R) -> np.ndarray:
    """The three pose angles in DEGREES of a rotation matrix: the inverse of render.euler_to_matrix for |rot[1]| < 90."""
    m = np.asarray(R, dtype=np.float64).reshape(3, 3)
    return np.degrees(np.array([np.arctan2(m[0, 1], m[0, 0]), np.arcsin(np.clip(m[0, 2], -1.0, 1.0)), np.arctan2(-m[1, 2], m[2, 2])]))


def rms(record) -> float:
    """Root mean square point-to-plane residual (mm) of a dh_fit_record; nan when no point was used."""
    n = int(record["points"])
    return float(np.sqrt(int(record["sum_r2_fixed"]) / 1048576.0 / n)) if n else float("nan")


def instances_from_poses(poses_or_heads, scale: float = 1.0, frames=None, model: int = 0) -> np.ndarray:
    """Start instances from dh_pose (POSE_DTYPE) or dh_head (HEAD_DTYPE) records: t = mid_point, R = euler_to_matrix of the
    record's rotation (radians in the record).  Record i belongs to frame i unless `frames` names each one's."""
    rec = np.asarray(poses_or_heads)
    if rec.dtype.names and "pose" in rec.dtype.names:
        rec = rec["pose"]
    rec = rec.reshape(-1)
    out = np.zeros(len(rec), dtype=RENDER_INSTANCE_DTYPE)
    for i, p in enumerate(rec):
        out[i] = (i if frames is None else int(frames[i]), model, euler_to_matrix(np.degrees(p["rotation"])).reshape(9),
                  p["mid_point"], scale, 0)
    return out


class Model(_lib._Handle):
    """One dh_fit_model: points [n, 3] (mm) and unit normals [n, 3] on `device`."""
    _handles = (("_h", "dh_fit_model_destroy"),)

    def __init__(self, points, normals, device: int = 0):
        self._lib = _lib.load()
        self.points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if self.points.shape != self.normals.shape:
            raise ValueError("as many normals as points are expected")
        self.device = int(device)
        self._h = C.c_void_p()
        check(self._lib.dh_fit_model_create(vp(self.points), vp(self.normals), C.c_uint32(len(self.points)), self.device, C.byref(self._h)))

    @classmethod
    def from_mesh(cls, verts, tris, device: int = 0) -> "Model":
        return cls(verts, vertex_normals(verts, tris), device=device)

    def info(self):
        """(n, radius = the largest |v|) as the library holds them."""
        n, radius = C.c_uint32(), C.c_double()
        check(self._lib.dh_fit_model_info(self._h, C.byref(n), C.byref(radius)))
        return n.value, radius.value


def views_from_rig(R, t):
    """The world-to-camera transforms (V [n, 3, 3] f32, u [n, 3] f32) of a rig's camera-to-world extrinsics R [n, 3, 3] (or
    [n, 9]) and t [n, 3], as `tracking.Rig` takes them: V = R^T, u = -(R^T t), in f64, rounded to f32 once.  ValueError when an
    R is not within DH_FIT_VIEW_TOLERANCE of a rotation (an element of R R^T off the identity's, or a determinant below 0)."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    if len(R) != len(t):
        raise ValueError("as many translations as rotations are expected")
    for c, r in enumerate(R):
        if not np.isfinite(r).all() or not (np.abs(r @ r.T - np.eye(3)) <= FIT_VIEW_TOLERANCE).all() or np.linalg.det(r) < 0.0:
            raise ValueError(f"camera {c}: R is not a rotation")
    V = np.transpose(R, (0, 2, 1))
    u = -np.einsum("nij,nj->ni", V, t)
    return np.ascontiguousarray(V, dtype=np.float32), np.ascontiguousarray(u, dtype=np.float32)


class Views(_lib._Handle):
    """One dh_fit_views: the world-to-camera transform (V [n, 3, 3], u [n, 3] mm) of every camera of
    `cameras` (a `tracking.Cameras`, which must outlive it), on that table's device: camera point = V x + u."""
    _handles = (("_h", "dh_fit_views_destroy"),)

    def __init__(self, cameras, V, u):
        self._lib = _lib.load()
        self.cameras = cameras
        self.V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3, 3)
        self.u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 3)
        if len(self.V) != len(cameras) or len(self.u) != len(cameras):
            raise ValueError("one V and one u per camera of the table are expected")
        self._h = C.c_void_p()
        check(self._lib.dh_fit_views_create(cameras._h, vp(self.V), vp(self.u), C.byref(self._h)))

    def __len__(self):
        return len(self.V)

    def info(self):
        """(n cameras, device) as the library holds them."""
        n, device = C.c_int(), C.c_int()
        check(self._lib.dh_fit_views_info(self._h, C.byref(n), C.byref(device)))
        return n.value, device.value


def view_instances_from_persons(persons, heads, rig_R, rig_t, rig_begin, scale: float = 1.0, model: int = 0) -> np.ndarray:
    """Start instances (VIEW_INSTANCE_DTYPE) of a multi-view fit from one rig's persons, as `tracking.RigTracker.step` reports
    them: `persons` the RIG_PERSON_DTYPE records of rig g, `heads` the step's HEAD_DTYPE [cameras, max_heads], rig_R / rig_t the
    extrinsics of all cameras and `rig_begin` the rig's first camera.  t is the person's `world`; R is rig_R[best_cam] times the
    best head's rotation, composed by tracking.world_rotation (best_cam indexes the whole camera table); views come from the
    person record and first_cam is `rig_begin` (rig_t is taken so that the call reads as the rig's; `world` already is in the
    world frame).  A host helper outside the bit-exact contract, as instances_from_poses is."""
    from .tracking import world_rotation
    persons = np.asarray(persons).reshape(-1)
    rig_R = np.asarray(rig_R, dtype=np.float64).reshape(-1, 3, 3)
    out = np.zeros(len(persons), dtype=VIEW_INSTANCE_DTYPE)
    for i, p in enumerate(persons):
        cam = int(p["best_cam"])
        R = world_rotation(rig_R[cam], heads[cam][int(p["best_head"])]["pose"]["rotation"])
        out[i] = (int(rig_begin), model, int(p["views"]), R.astype(np.float32).reshape(9), p["world"], scale, 0)
    return out


class ShapeBasis(_lib._Handle):
    """One dh_fit_basis: K displacement fields [K, n, 3] (mm) of a model of n points, on `device`."""
    _handles = (("_h", "dh_fit_basis_destroy"),)

    def __init__(self, fields, device: int = 0):
        self._lib = _lib.load()
        self.fields = np.ascontiguousarray(fields, dtype=np.float32)
        if self.fields.ndim != 3 or self.fields.shape[2] != 3:
            raise ValueError("fields [K, n, 3] are expected")
        self.device = int(device)
        self._h = C.c_void_p()
        check(self._lib.dh_fit_basis_create(vp(self.fields), C.c_uint32(self.fields.shape[1]), C.c_uint32(self.fields.shape[0]), self.device,
                                            C.byref(self._h)))

    def __len__(self):
        return self.fields.shape[0]

    def info(self):
        """(n, K, the largest |B_k[i]|) as the library holds them."""
        n, k, largest = C.c_uint32(), C.c_uint32(), C.c_double()
        check(self._lib.dh_fit_basis_info(self._h, C.byref(n), C.byref(k), C.byref(largest)))
        return n.value, k.value, largest.value


def _params(struct, default: str, **fields):
    """A `struct` as the library's `default` function fills it, with every field given (not None) replaced: cast by the field's
    own ctypes type -- doubles with float, integers with int, an array element by element (as many values as it has elements)."""
    p = struct()
    check(getattr(_lib.load(), default)(C.byref(p)))
    types = dict(struct._fields_)
    for name, value in fields.items():
        if value is None:
            continue
        t = types[name]
        if issubclass(t, C.Array):
            cast = float if t._type_ is C.c_double else int
            getattr(p, name)[:] = [cast(v) for v in value]
        else:
            setattr(p, name, float(value) if t is C.c_double else int(value))
    return p


def shape_params(gate=None, lam=None, min_points=None) -> "_lib.ShapeParams":
    """dh_shape_params_default with the given fields replaced."""
    return _params(_lib.ShapeParams, "dh_shape_params_default", gate=gate, lam=lam, min_points=min_points)


def surface_params(gate=None, min_cos2=None, mu=None, eps=None, min_count=None, min_points=None, iterations=None) -> "_lib.SurfaceParams":
    """dh_fit_surface_params_default with the given fields replaced."""
    return _params(_lib.SurfaceParams, "dh_fit_surface_params_default", gate=gate, min_cos2=min_cos2, mu=mu, eps=eps, min_count=min_count,
                   min_points=min_points, iterations=iterations)


def ident_params(iterations=None, min_points=None, gate=None, lam=None, max_rms=None, min_ratio=None) -> "_lib.IdentParams":
    """dh_fit_ident_params_default with the given fields replaced."""
    return _params(_lib.IdentParams, "dh_fit_ident_params_default", iterations=iterations, min_points=min_points, gate=gate, lam=lam, max_rms=max_rms,
                   min_ratio=min_ratio)


def ident_views_params(iterations=None, min_points=None, gate=None, lam=None, max_rms=None, min_ratio=None) -> "_lib.IdentParams":
    """dh_fit_ident_views_params_default -- the multi-view call's own measured max_rms -- with the given fields replaced."""
    return _params(_lib.IdentParams, "dh_fit_ident_views_params_default", iterations=iterations, min_points=min_points, gate=gate, lam=lam,
                   max_rms=max_rms, min_ratio=min_ratio)


def calib_params(gate=None, lam=None, min_points=None, pivot=None) -> "_lib.CalibParams":
    """dh_calib_params_default with the given fields replaced."""
    return _params(_lib.CalibParams, "dh_calib_params_default", gate=gate, lam=lam, min_points=min_points, pivot=pivot)


def views_from_records(cameras, views_V, views_u, records) -> "Views":
    """The next view table after a calibration step: a new `Views` of `cameras` that takes V and u from
    every record whose status is CALIB_OK and keeps the old entry (views_V [n, 3, 3], views_u [n, 3]) elsewhere.  A
    dh_fit_views is immutable, so each round makes a new table on the host; the old one may be closed once nothing is bound to
    it."""
    V = np.array(views_V, dtype=np.float32).reshape(-1, 3, 3)
    u = np.array(views_u, dtype=np.float32).reshape(-1, 3)
    rec = np.asarray(records).reshape(-1)
    if len(rec) != len(V) or len(u) != len(V):
        raise ValueError("one record, one V and one u per camera are expected")
    ok = rec["status"] == CALIB_OK
    V[ok] = rec["V"][ok].reshape(-1, 3, 3)
    u[ok] = rec["u"][ok]
    return Views(cameras, V, u)


def deform(verts, basis, coeffs) -> np.ndarray:
    """The deformed vertices [n, 3] f32: v_i + sum_k c_k B_k[i] in f64, the fields added in index order, rounded to f32 once.
    `basis` is a ShapeBasis or its fields [K, n, 3]."""
    B = np.asarray(getattr(basis, "fields", basis), dtype=np.float32).astype(np.float64)
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    c = np.asarray(coeffs, dtype=np.float64).reshape(-1)
    if B.shape[1:] != v.shape or len(c) != len(B):
        raise ValueError("basis [K, n, 3], verts [n, 3] and K coefficients are expected")
    for k in range(len(B)):
        v = v + c[k] * B[k]
    return v.astype(np.float32)


def fit_params(coarse_iterations=None, iterations=None, gate=None, lam=None, min_points=None) -> "_lib.FitParams":
    """dh_fit_params_default with the given fields replaced."""
    return _params(_lib.FitParams, "dh_fit_params_default", coarse_iterations=coarse_iterations, iterations=iterations, gate=gate, lam=lam,
                   min_points=min_points)


_RECORD_NAMES = {FIT_RECORD_DTYPE: "dh_fit_record", VIEW_FIT_RECORD_DTYPE: "dh_view_fit_record"}


def check_tensor(t, device, name, dtype=None, count=None, per="instance"):
    """ValueError, in the words of argument `name`, unless the torch tensor `t` can go to a _device form as a device address:
    it lies on `device` (a torch.device), is contiguous and, where `count` is given, is `count` items of `dtype` long -- in
    elements of the dtype's own size for a plain dtype (the frames, the word and the byte arrays), of any size for a record
    dtype.  `per` is what the message says there is one item of.  Needs no fitter and no GPU."""
    dtype = None if dtype is None else np.dtype(dtype)
    plain = dtype is not None and dtype.names is None
    if (t.device == device and t.is_contiguous() and (not plain or t.element_size() == dtype.itemsize)
            and (count is None or t.numel() * t.element_size() == count * dtype.itemsize)):
        return
    if name == "frames":
        raise ValueError("device frames: a contiguous 16-bit tensor on the fitter's device is expected")
    if name == "instances":
        raise ValueError("device instances: a contiguous tensor on the fitter's device is expected")
    if name == "carried":
        raise ValueError("carried: the contiguous device tensor of an earlier fit of as many instances is expected")
    if plain:
        raise ValueError(f"device {name}: a contiguous {8 * dtype.itemsize}-bit tensor with one {'word' if dtype.itemsize == 4 else 'byte'} "
                         f"per {per} is expected")
    raise ValueError(f"device {name}: the contiguous tensor of one {_RECORD_NAMES[dtype]} per {per} is expected")


_U8, _U16, _U32 = np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.uint32)
_DEVICES = {}       # ordinal -> (torch, torch.device("cuda", ordinal)), filled by the first _device form of a fitter on it


class _Call:
    """The arguments of one call of a Fitter, bound for its host form or its _device form.  The method
    writes the C call once, `call(name, argument, ...)` in the header's order after the fitter's handle, and gets each array
    argument from one of the methods below; Python evaluates them from left to right, so every refusal comes in the header's
    order and before the first output is allocated.  Host form: numpy arrays in and out, each input kept alive by its
    pointer.  _device form: torch tensors on the fitter's device, checked by `check_tensor`, and the stream as the last
    argument.  After `instances`, `ni` is their count."""
    dev, ni, infix = None, 0, ""

    def __init__(self, fitter, device_out: bool, stream):
        self.fitter, self.stream, self.outs = fitter, stream, []
        if device_out:
            if fitter.device not in _DEVICES:
                import torch
                _DEVICES[fitter.device] = torch, torch.device("cuda", fitter.device)
            self.torch, self.dev = _DEVICES[fitter.device]

    def frames(self, frames):
        if self.dev is None:
            return _lib.held(np.ascontiguousarray(frames, dtype=_U16))
        check_tensor(frames, self.dev, "frames", _U16)
        return C.c_void_p(frames.data_ptr())

    def instances(self, instances, dtype, host: bool = False):
        """The instances, NULL when there are none; host=True: a numpy array in both forms."""
        if self.dev is None or host:
            inst = np.ascontiguousarray(instances, dtype=dtype)
            self.ni = len(inst)
            return _lib.held(inst) if self.ni else None
        check_tensor(instances, self.dev, "instances")
        self.ni = instances.numel() * instances.element_size() // dtype.itemsize
        return C.c_void_p(instances.data_ptr()) if self.ni else None

    def inp(self, name, array, dtype, count, per="instance", nonzero: bool = False):
        """A nullable input of `count` items of `dtype`, one per `per`: None binds NULL.  nonzero=True: bytes that the host form
        normalises with != 0."""
        if array is None:
            return None
        if self.dev is None:
            return _lib.held(np.ascontiguousarray(np.asarray(array) != 0 if nonzero else array, dtype=dtype).reshape(max(count, 0)))
        check_tensor(array, self.dev, name, dtype, count, per)
        return C.c_void_p(array.data_ptr())

    def carried(self, carried, dtype):
        """The instances an earlier fit left on the device, to be spliced into the list with `*`: an argument of the _device
        form alone, and only when given -- the call's name then gets `_carried`."""
        if carried is None or self.dev is None:
            return ()
        check_tensor(carried, self.dev, "carried", dtype, self.ni)
        self.infix = "_carried"
        return (C.c_void_p(carried.data_ptr()) if self.ni else None,)

    def out(self, dtype, *shape, fill=0, give: bool = True, spare: int = 1):
        """An output of `shape` items of `dtype`; give=False: NULL, and the call returns nothing for it.  Host form: a numpy
        array of `fill`.  _device form: a flat torch tensor -- int32 for words, else the records' bytes as uint8 -- of at least
        `spare` items, cut to the items asked for (no empty allocation: its address would be NULL)."""
        if not give:
            return None
        if self.dev is None:
            shape = tuple([max(s, 0) for s in shape])
            self.outs.append(np.full(shape, fill, dtype) if fill else np.zeros(shape, dtype))
            return vp(self.outs[-1])
        count = math.prod(shape)
        size, kind = (1, self.torch.int32) if dtype.names is None else (dtype.itemsize, self.torch.uint8)
        t = self.torch.empty(max(count, spare) * size, dtype=kind, device=self.dev)
        self.outs.append(t if count >= spare else t[:count * size])     # (cut only where the spare item was allocated)
        return C.c_void_p(t.data_ptr())

    def call(self, name, *args):
        """Call `name` -- `name` + `_device` with the stream appended in that form -- and return the outputs in the order they
        were declared: one as itself, several as a tuple."""
        f = self.fitter
        if self.dev is None:
            check(getattr(f._lib, name)(f._h, *args))
        else:
            check(getattr(f._lib, name + self.infix + "_device")(f._h, *args, C.c_void_p(_lib.stream_of(self.dev, self.stream))))
        return self.outs[0] if len(self.outs) == 1 else tuple(self.outs)


class Fitter(_lib._Handle):
    """One dh_fitter on `device`.  Not thread-safe."""
    _handles = (("_h", "dh_fitter_destroy"),)

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        self.device = int(device)
        self._h = C.c_void_p()
        check(self._lib.dh_fitter_create(self.device, C.byref(self._h)))

    def fit(self, frames, models, instances, K_or_cameras, params=None, device_out: bool = False, stream=None, carried=None):
        """Refine `instances` (a RENDER_INSTANCE_DTYPE array of rough poses) of `models` against `frames`: [n, h, w] u16 as a
        numpy array, or a torch tensor on the device with device_out=True.  Through one K ([3, 3] or an `IntrinsicMatrix`) or a
        `tracking.Cameras` table of exactly n cameras.  Returns (instances, records) -- RENDER_INSTANCE_DTYPE and
        FIT_RECORD_DTYPE arrays, or with device_out=True two uint8 torch tensors on the device holding them, ordered on `stream`
        (default the current torch stream).  `carried` (device_out=True only): the uint8 tensor an earlier fit(device_out=True)
        returned for the same instances, whose R and t the fit starts from in place of those of `instances` (DESIGN.md section
        25)."""
        models = list(models)
        handles = (C.c_void_p * max(len(models), 1))(*[m._h.value for m in models])
        n, h, w = (int(v) for v in frames.shape)
        kind, karg = _lib.intrinsics(K_or_cameras)
        b = _Call(self, device_out, stream)
        return b.call("dh_fit_depth" + kind, b.frames(frames), n, w, h, karg, handles, C.c_uint32(len(models)),
                      b.instances(instances, RENDER_INSTANCE_DTYPE, host=True), C.c_uint32(b.ni), *b.carried(carried, RENDER_INSTANCE_DTYPE),
                      _lib.ref(params), b.out(RENDER_INSTANCE_DTYPE, b.ni), b.out(FIT_RECORD_DTYPE, b.ni))

    def fit_views(self, frames, models, instances, views, params=None, device_out: bool = False, stream=None):
        """Fit each of `instances` (VIEW_INSTANCE_DTYPE: one world pose and the mask of the cameras that see it) against the
        frames of all its views at once.  frames [n, h, w] u16, frame c seen through camera c of `views`
        (a `Views` of n cameras): a numpy array, or a torch tensor on the device with device_out=True.  Returns (instances,
        records) -- VIEW_INSTANCE_DTYPE and VIEW_FIT_RECORD_DTYPE arrays, or with device_out=True two uint8 torch tensors on the
        device holding them, ordered on `stream` (default the current torch stream)."""
        models = list(models)
        handles = (C.c_void_p * max(len(models), 1))(*[m._h.value for m in models])
        n, h, w = (int(v) for v in frames.shape)
        if n != len(views):
            raise ValueError(f"{n} frames for a view table of {len(views)} cameras")
        b = _Call(self, device_out, stream)
        return b.call("dh_fit_depth_views", b.frames(frames), w, h, views._h, handles, C.c_uint32(len(models)),
                      b.instances(instances, VIEW_INSTANCE_DTYPE, host=True), C.c_uint32(b.ni), _lib.ref(params),
                      b.out(VIEW_INSTANCE_DTYPE, b.ni), b.out(VIEW_FIT_RECORD_DTYPE, b.ni))

    def shape_step(self, frames, model, basis, instances, K_or_cameras, subjects=None, n_subjects: int = 1, params=None,
                   device_out: bool = False, stream=None):
        """One shape step of `model` and its `basis` over the fitted `instances` of `frames`, per subject:
        subjects [n_instances] u32 (None: all subject 0; SHAPE_SKIP leaves an instance out).  Host form: numpy frames and
        instances -> SHAPE_RECORD_DTYPE [n_subjects].  With device_out=True frames, instances and subjects are torch tensors on
        the device (instances as the uint8 tensor Fitter.fit(device_out=True) returned, subjects int32 or None) and the records
        come back as a uint8 torch tensor, ordered on `stream` (default the current torch stream) without a host wait."""
        n, h, w = (int(v) for v in frames.shape)
        kind, karg = _lib.intrinsics(K_or_cameras)
        ns = int(n_subjects)
        b = _Call(self, device_out, stream)
        return b.call("dh_fit_shape" + kind, b.frames(frames), n, w, h, karg, model._h, basis._h, b.instances(instances, RENDER_INSTANCE_DTYPE),
                      C.c_uint32(b.ni), b.inp("subjects", subjects, _U32, b.ni), C.c_uint32(ns), _lib.ref(params),
                      b.out(SHAPE_RECORD_DTYPE, ns))

    def shape_step_subjects(self, frames, subjects_set, instances, K_or_cameras, subjects=None, n_subjects=None, fit_records=None, params=None,
                            device_out: bool = False, stream=None):
        """`shape_step` over a `Subjects` set: instance i is taken at the model of subject subjects[i] (None:
        subject 0), and where `fit_records` (FIT_RECORD_DTYPE [n_instances], what `fit` returned with the instances) is given,
        an instance whose fit did not end FIT_OK takes no part.  n_subjects defaults to the set's.  Host form: numpy arrays ->
        SHAPE_RECORD_DTYPE [n_subjects].  With device_out=True frames, instances, subjects and fit_records are torch tensors on
        the device (instances and fit_records as the uint8 tensors Fitter.fit(device_out=True) returned, subjects int32 or None)
        and the records come back as a uint8 torch tensor, ordered on `stream` without a host wait."""
        return self._step_subjects("dh_fit_shape_subjects", SHAPE_RECORD_DTYPE, frames, subjects_set, instances, K_or_cameras, subjects, n_subjects,
                                   fit_records, params, device_out, stream)

    def surface_step_subjects(self, frames, subjects_set, instances, K_or_cameras, subjects=None, n_subjects=None, fit_records=None, params=None,
                              device_out: bool = False, stream=None):
        """One surface step over a `Subjects` set made with max_offset: every offset of subjects
        0 .. n_subjects - 1 re-estimated from the fitted `instances`, and their models evaluated.  The arguments are
        `shape_step_subjects`'s.  Host form: numpy arrays -> SURFACE_RECORD_DTYPE [n_subjects].  With device_out=True frames,
        instances, subjects and fit_records are torch tensors on the device and the records come back as a uint8 torch tensor:
        five kernels ordered on `stream`, no host wait."""
        return self._step_subjects("dh_fit_surface_subjects", SURFACE_RECORD_DTYPE, frames, subjects_set, instances, K_or_cameras, subjects,
                                   n_subjects, fit_records, params, device_out, stream)

    def _step_subjects(self, name, record, frames, subjects_set, instances, K_or_cameras, subjects, n_subjects, fit_records, params, device_out,
                       stream):
        """The shape step and the surface step over a subject set: one argument list, two calls and record types."""
        n, h, w = (int(v) for v in frames.shape)
        kind, karg = _lib.intrinsics(K_or_cameras)
        ns = len(subjects_set) if n_subjects is None else int(n_subjects)
        b = _Call(self, device_out, stream)
        return b.call(name + kind, b.frames(frames), n, w, h, karg, subjects_set._h, b.instances(instances, RENDER_INSTANCE_DTYPE), C.c_uint32(b.ni),
                      b.inp("subjects", subjects, _U32, b.ni), C.c_uint32(ns), b.inp("fit_records", fit_records, FIT_RECORD_DTYPE, b.ni),
                      _lib.ref(params), b.out(record, ns))

    def identify_subjects(self, frames, subjects_set, instances, K_or_cameras, n_subjects=None, enrolled=None, fit_records=None, params=None,
                          scores: bool = False, device_out: bool = False, stream=None):
        """Which enrolled subject of a `Subjects` set each fitted instance is: every instance that takes
        part is refitted with the model of every candidate -- the subjects s < n_subjects (default the set's) with enrolled[s] != 0
        (None: all) -- and the candidate with the smallest mean squared residual wins, unless it exceeds params.max_rms (IDENT_FAR)
        or the second is within params.min_ratio of it (IDENT_AMBIGUOUS).  `fit_records` (what `fit` returned with the instances)
        leaves out an instance whose fit did not end FIT_OK.  Returns (subjects u32 [n_instances] -- IDENT_UNKNOWN, which is
        SHAPE_SKIP, where the status is not IDENT_OK --, IDENT_RECORD_DTYPE records, the instances with the best candidate's
        refitted pose) and, with scores=True, every pair's FIT_RECORD_DTYPE [n_instances, n_subjects] after them.  Host form: numpy
        arrays.  With device_out=True frames, instances, enrolled (uint8) and fit_records are torch tensors on the device and the
        results come back as torch tensors (subjects int32, the others uint8): two kernels ordered on `stream`, no host wait."""
        n, h, w = (int(v) for v in frames.shape)
        kind, karg = _lib.intrinsics(K_or_cameras)
        ns = len(subjects_set) if n_subjects is None else int(n_subjects)
        b = _Call(self, device_out, stream)
        return b.call("dh_fit_identify_subjects" + kind, b.frames(frames), n, w, h, karg, subjects_set._h, b.instances(instances, RENDER_INSTANCE_DTYPE),
                      C.c_uint32(b.ni), b.inp("enrolled", enrolled, _U8, ns, per="subject", nonzero=True), C.c_uint32(ns),
                      b.inp("fit_records", fit_records, FIT_RECORD_DTYPE, b.ni), _lib.ref(params), b.out(_U32, b.ni, fill=IDENT_UNKNOWN),
                      b.out(IDENT_RECORD_DTYPE, b.ni), b.out(RENDER_INSTANCE_DTYPE, b.ni), b.out(FIT_RECORD_DTYPE, b.ni, ns, give=scores))

    def shape_step_views(self, frames, views, model, basis, instances, sets=None, subjects=None, n_subjects: int = 1, params=None,
                         device_out: bool = False, stream=None):
        """One multi-view shape step of `model` and its `basis` over the world-posed `instances`
        (VIEW_INSTANCE_DTYPE, what fit_views returned) of frames [n_sets, n, h, w] u16 -- frame [s, c] is camera c of `views` (a
        `Views` of n cameras) at set s -- per subject: sets [n_instances] u32 (None: all in set 0), subjects [n_instances] u32
        (None: all subject 0; SHAPE_SKIP leaves an instance out).  The record's `instances` counts (instance, view) pairs.  Host
        form: numpy arrays -> SHAPE_RECORD_DTYPE [n_subjects].  With device_out=True frames, instances, sets and subjects are
        torch tensors on the device (instances as the uint8 tensor Fitter.fit_views(device_out=True) returned, sets and subjects
        int32 or None) and the records come back as a uint8 torch tensor, ordered on `stream` (default the current torch stream)
        without a host wait."""
        n_sets, n, h, w = (int(v) for v in frames.shape)
        if n != len(views):
            raise ValueError(f"{n} frames a set for a view table of {len(views)} cameras")
        ns = int(n_subjects)
        b = _Call(self, device_out, stream)
        return b.call("dh_fit_shape_views", b.frames(frames), C.c_uint32(n_sets), w, h, views._h, model._h, basis._h,
                      b.instances(instances, VIEW_INSTANCE_DTYPE), C.c_uint32(b.ni), b.inp("sets", sets, _U32, b.ni),
                      b.inp("subjects", subjects, _U32, b.ni), C.c_uint32(ns), _lib.ref(params), b.out(SHAPE_RECORD_DTYPE, ns))

    def identify_subjects_views(self, frames, views, subjects_set, instances, sets=None, n_subjects=None, enrolled=None, fit_records=None,
                                params=None, scores: bool = False, device_out: bool = False, stream=None):
        """Which enrolled subject of a `Subjects` set each world-posed instance is, decided from all the cameras that see it
        (DESIGN.md section 28): `identify_subjects` with the multi-view fit for the score.  frames [n_sets, n, h, w] u16 -- frame
        [s, c] is camera c of `views` (a `Views` of n cameras) at set s; instances VIEW_INSTANCE_DTYPE (what fit_views returned),
        sets [n_instances] u32 (None: all in set 0), fit_records VIEW_FIT_RECORD_DTYPE (what fit_views returned with them).
        params None selects the multi-view defaults (`ident_views_params`).  Returns (subjects u32 [n_instances], IDENT_RECORD_DTYPE
        records, the instances with the best candidate's refitted world pose) and, with scores=True, every pair's
        VIEW_FIT_RECORD_DTYPE [n_instances, n_subjects] after them.  Host form: numpy arrays.  With device_out=True frames,
        instances, sets (int32), enrolled (uint8) and fit_records are torch tensors on the device and the results come back as torch
        tensors (subjects int32, the others uint8): two kernels ordered on `stream`, no host wait.  All identify calls of one
        fitter must be ordered on one stream."""
        n_sets, n, h, w = (int(v) for v in frames.shape)
        if n != len(views):
            raise ValueError(f"{n} frames a set for a view table of {len(views)} cameras")
        ns = len(subjects_set) if n_subjects is None else int(n_subjects)
        b = _Call(self, device_out, stream)
        return b.call("dh_fit_identify_subjects_views", b.frames(frames), C.c_uint32(n_sets), w, h, views._h, subjects_set._h,
                      b.instances(instances, VIEW_INSTANCE_DTYPE), C.c_uint32(b.ni), b.inp("sets", sets, _U32, b.ni),
                      b.inp("enrolled", enrolled, _U8, ns, per="subject", nonzero=True), C.c_uint32(ns),
                      b.inp("fit_records", fit_records, VIEW_FIT_RECORD_DTYPE, b.ni), _lib.ref(params), b.out(_U32, b.ni, fill=IDENT_UNKNOWN),
                      b.out(IDENT_RECORD_DTYPE, b.ni), b.out(VIEW_INSTANCE_DTYPE, b.ni), b.out(VIEW_FIT_RECORD_DTYPE, b.ni, ns, give=scores))

    def calibrate_step(self, frames, views, model, instances, sets=None, take=None, hold=None, params=None, device_out: bool = False,
                       stream=None):
        """One calibration step of the cameras of `views` (a `Views` of n cameras) over the world-posed
        `instances` (VIEW_INSTANCE_DTYPE, what fit_views returned) of frames [n_sets, n, h, w] u16, with `model` held: sets
        [n_instances] u32 (None: all in set 0), take [n_instances] u32 (None: all take part; CALIB_SKIP leaves an instance out),
        hold [n] u8 (None: none; non-zero: the camera is held and gets no update).  Host form: numpy arrays -> CALIB_RECORD_DTYPE
        [n], one record per camera.  With device_out=True frames, instances, sets, take and hold are torch tensors on the device
        (instances as the uint8 tensor Fitter.fit_views(device_out=True) returned, sets and take int32 or None, hold uint8 or
        None) and the records come back as a uint8 torch tensor, ordered on `stream` (default the current torch stream) without
        a host wait."""
        n_sets, n, h, w = (int(v) for v in frames.shape)
        if n != len(views):
            raise ValueError(f"{n} frames a set for a view table of {len(views)} cameras")
        b = _Call(self, device_out, stream)
        return b.call("dh_fit_calibrate_views", b.frames(frames), C.c_uint32(n_sets), w, h, views._h, model._h,
                      b.instances(instances, VIEW_INSTANCE_DTYPE), C.c_uint32(b.ni), b.inp("sets", sets, _U32, b.ni),
                      b.inp("take", take, _U32, b.ni), b.inp("hold", hold, _U8, n, per="camera"), _lib.ref(params),
                      b.out(CALIB_RECORD_DTYPE, n, spare=0))


def adapt(fitter, frames, K_or_cameras, verts, tris, basis, starts, rounds: int = 6, fit_prm=None, shape_prm=None, coeffs=None):
    """Adapt the shape coefficients of one subject's model to `frames` ([n, h, w] u16, numpy) by alternation, `rounds` times:
    build the model from the current coefficients (deform, vertex_normals); fit every frame from its previous pose (the first
    round from `starts`, RENDER_INSTANCE_DTYPE [m]); take one shape step over the fits that ended FIT_OK; add the increment
    when the step ended SHAPE_OK.  Each round waits on the host: this happens once per subject, not once per frame.  `basis` is
    the fields [K, n, 3] of the undeformed `verts`.  Returns (coefficients [K] f64, the last fitted instances, trace): trace[r]
    holds the round's coefficients before the step, the fit records, the shape record and the increment."""
    fields = np.ascontiguousarray(getattr(basis, "fields", basis), dtype=np.float32)
    c = np.zeros(len(fields), np.float64) if coeffs is None else np.array(coeffs, dtype=np.float64)
    inst = np.array(starts, dtype=RENDER_INSTANCE_DTYPE)
    trace = []
    with ShapeBasis(fields, device=fitter.device) as sb:
        for _ in range(int(rounds)):
            v = deform(verts, fields, c)
            with Model(v, vertex_normals(v, tris), device=fitter.device) as model:
                inst, rec = fitter.fit(frames, [model], inst, K_or_cameras, params=fit_prm)
                subj = np.where(rec["status"] == FIT_OK, 0, SHAPE_SKIP).astype(np.uint32)
                srec = fitter.shape_step(frames, model, sb, inst, K_or_cameras, subjects=subj, params=shape_prm)[0]
            delta = srec["delta"][:len(c)].copy() if srec["status"] == SHAPE_OK else np.zeros(len(c))
            trace.append({"coeffs": c.copy(), "fit": rec, "shape": srec, "delta": delta})
            c = c + delta
    return c, inst, trace

class _SetModel:
    """One model of a `Subjects` set: what Fitter's calls and the trackers read of a `Model` (its handle), borrowed -- the set owns it."""

    def __init__(self, lib, handle, device):
        self._lib, self._h, self.device = lib, handle, device

    def info(self):
        """(n, radius): the radius is the set's bound on every model it can hold."""
        n, radius = C.c_uint32(), C.c_double()
        check(self._lib.dh_fit_model_info(self._h, C.byref(n), C.byref(radius)))
        return n.value, radius.value


class Subjects(_lib._Handle):
    """One dh_fit_subjects: `n_subjects` deformable models of the mesh (verts [n, 3], tris [m, 3]) on
    `device`, each with its own coefficients of `basis` (a `ShapeBasis` of n points, which must outlive the set), every
    coefficient kept within +-max_coeff.  `models[s]` is subject s's model for any call that takes a `Model`; its contents
    follow the subject's coefficients with every `update`."""
    _handles = (("_h", "dh_fit_subjects_destroy"),)

    def __init__(self, verts, tris, basis, n_subjects: int, max_coeff: float = 0.5, device: int = 0, max_offset=None):
        """max_offset (mm; None: none): a SURFACE set, which also holds one offset per (subject, vertex)
        along the base mesh's vertex normal, each kept within +-max_offset, for `Fitter.surface_step_subjects`."""
        self._lib = _lib.load()
        self.verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        self.tris = np.ascontiguousarray(tris, dtype=np.uint32).reshape(-1, 3)
        self.basis, self.device, self.n_subjects, self.max_coeff = basis, int(device), int(n_subjects), float(max_coeff)
        self.max_offset = None if max_offset is None else float(max_offset)
        self._h = C.c_void_p()
        if self.max_offset is None:
            check(self._lib.dh_fit_subjects_create(vp(self.verts), C.c_uint32(len(self.verts)), vp(self.tris), C.c_uint32(len(self.tris)), basis._h,
                                                   C.c_uint32(self.n_subjects), C.c_double(self.max_coeff), self.device, C.byref(self._h)))
        else:
            check(self._lib.dh_fit_subjects_create_surface(vp(self.verts), C.c_uint32(len(self.verts)), vp(self.tris), C.c_uint32(len(self.tris)),
                                                           basis._h, C.c_uint32(self.n_subjects), C.c_double(self.max_coeff),
                                                           C.c_double(self.max_offset), self.device, C.byref(self._h)))
        self.models = []
        for s in range(self.n_subjects):
            h = C.c_void_p()
            check(self._lib.dh_fit_subjects_model(self._h, C.c_uint32(s), C.byref(h)))
            self.models.append(_SetModel(self._lib, h, self.device))

    def __len__(self):
        return self.n_subjects

    def close(self):
        self.models = []
        super().close()

    def info(self):
        """(n, n_tris, K, S, the radius bound, device) as the library holds them."""
        n, nt, k, s, radius, device = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_double(), C.c_int()
        check(self._lib.dh_fit_subjects_info(self._h, C.byref(n), C.byref(nt), C.byref(k), C.byref(s), C.byref(radius), C.byref(device)))
        return n.value, nt.value, k.value, s.value, radius.value, device.value

    def state(self) -> np.ndarray:
        """Synchronous copy of the subjects' states: SUBJECT_STATE_DTYPE [S]."""
        st = np.zeros(self.n_subjects, SUBJECT_STATE_DTYPE)
        check(self._lib.dh_fit_subjects_state(self._h, vp(st)))
        return st

    def read(self, subject: int):
        """Synchronous copy of subject `subject`'s model as it stands: (points [n, 3] f32, normals [n, 3] f32)."""
        pts, nrm = np.zeros_like(self.verts), np.zeros_like(self.verts)
        check(self._lib.dh_fit_subjects_read(self._h, C.c_uint32(int(subject)), vp(pts), vp(nrm)))
        return pts, nrm

    def set_coeffs(self, coeffs, first: int = 0) -> None:
        """Set the coefficients of subjects first .. first + len(coeffs) - 1 (coeffs [count, K] or [count, 8]) and evaluate their
        models; synchronous."""
        c = np.asarray(coeffs, dtype=np.float64)
        c = c.reshape(-1, c.shape[-1])
        full = np.zeros((len(c), 8), np.float64)
        full[:, :c.shape[1]] = c
        check(self._lib.dh_fit_subjects_set_coeffs(self._h, C.c_uint32(int(first)), C.c_uint32(len(full)), vp(full)))

    def offsets(self, subject: int, counts: bool = False):
        """Synchronous copy of subject `subject`'s offsets [n] f64 (a surface set); with counts=True (offsets, counts [n] u32): how
        often the last surface step saw each vertex."""
        o, c = np.zeros(len(self.verts), np.float64), np.zeros(len(self.verts), np.uint32)
        check(self._lib.dh_fit_subjects_read_offsets(self._h, C.c_uint32(int(subject)), vp(o), vp(c) if counts else None))
        return (o, c) if counts else o

    def set_offsets(self, subject: int, offsets) -> None:
        """Set subject `subject`'s offsets [n] (mm, each within +-max_offset) and evaluate its model; synchronous."""
        o = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        if len(o) != len(self.verts):
            raise ValueError("one offset per vertex is expected")
        check(self._lib.dh_fit_subjects_set_offsets(self._h, C.c_uint32(int(subject)), vp(o)))

    def update(self, records, device: bool = False, stream=None) -> None:
        """Apply one shape record per subject (SHAPE_RECORD_DTYPE [S], what shape_step_subjects returned) and evaluate every
        model.  Host form: a numpy array, synchronous.  device=True: the uint8 torch tensor of shape_step_subjects(device_out=True),
        three kernels on `stream` (default the current torch stream), no host wait."""
        if not device:
            rec = np.ascontiguousarray(records, dtype=SHAPE_RECORD_DTYPE).reshape(self.n_subjects)
            check(self._lib.dh_fit_subjects_update(self._h, vp(rec)))
            return
        if records.numel() * records.element_size() != self.n_subjects * SHAPE_RECORD_DTYPE.itemsize or not records.is_contiguous():
            raise ValueError("device records: the contiguous tensor of one dh_shape_record per subject is expected")
        check(self._lib.dh_fit_subjects_update_device(self._h, C.c_void_p(records.data_ptr()), C.c_void_p(_lib.stream_of(self.device, stream))))


def adapt_subjects(fitter, frames, K_or_cameras, subjects, starts, subject_of, rounds: int = 6, fit_prm=None, shape_prm=None):
    """`adapt` for all the subjects of a `Subjects` set at once, on the device.  frames [n, h, w] u16
    (numpy) go to the device once; `starts` are RENDER_INSTANCE_DTYPE [m] rough poses and subject_of [m] names each one's
    subject.  Every round is one fit of all instances -- instance i against models[subject_of[i]], from `starts` in the first
    round and from the previous round's fitted poses after it (`carried`) -- one shape step over the set with the fit's records
    as the filter, and one update of the set, all enqueued on the current torch stream: the host reads nothing inside the loop
    and once at the end.  The set's coefficients are adapted in place, from where they stand.  Returns (state
    SUBJECT_STATE_DTYPE [S], the last fitted instances, the FIT_RECORD_DTYPE and SHAPE_RECORD_DTYPE records of the last round)."""
    import torch
    dev = torch.device("cuda", fitter.device)
    inst = np.array(starts, dtype=RENDER_INSTANCE_DTYPE)
    who = np.ascontiguousarray(subject_of, dtype=np.uint32).reshape(len(inst))
    inst["mesh"] = who
    host = np.ascontiguousarray(frames, dtype=np.uint16)
    d_frames = torch.from_numpy((host if host.flags.writeable else host.copy()).view(np.int16)).to(dev)
    d_who = torch.from_numpy(who.view(np.int32)).to(dev)
    d_inst = d_frec = d_srec = None
    for _ in range(int(rounds)):
        d_inst, d_frec = fitter.fit(d_frames, subjects.models, inst, K_or_cameras, params=fit_prm, device_out=True, carried=d_inst)
        d_srec = fitter.shape_step_subjects(d_frames, subjects, d_inst, K_or_cameras, subjects=d_who, fit_records=d_frec, params=shape_prm,
                                            device_out=True)
        subjects.update(d_srec, device=True)
    torch.cuda.current_stream(dev).synchronize()
    if d_inst is None:
        return subjects.state(), inst, (np.zeros(len(inst), FIT_RECORD_DTYPE), np.zeros(len(subjects), SHAPE_RECORD_DTYPE))
    out = d_inst.cpu().numpy().view(RENDER_INSTANCE_DTYPE).copy()
    return subjects.state(), out, (d_frec.cpu().numpy().view(FIT_RECORD_DTYPE).copy(), d_srec.cpu().numpy().view(SHAPE_RECORD_DTYPE).copy())


def refine_subjects(fitter, frames, K_or_cameras, subjects, starts, subject_of, rounds: int = 6, shape_rounds: int = 0, fit_prm=None,
                    shape_prm=None, surface_prm=None):
    """Refine every subject of a surface `Subjects` set per vertex, on the device.  frames [n, h, w] u16
    (numpy) go to the device once; `starts` and subject_of are `adapt_subjects`'s.  Every round is one fit of all instances from
    the previous round's poses (`carried`); in the first `shape_rounds` rounds one shape step over the set and its update; then
    one surface step -- all enqueued on the current torch stream, nothing read inside the loop and once at the end.  Offsets
    and coefficients are refined in place, from where they stand.  Returns (state SUBJECT_STATE_DTYPE [S], the last fitted
    instances, the FIT_RECORD_DTYPE and SURFACE_RECORD_DTYPE records of the last round)."""
    import torch
    dev = torch.device("cuda", fitter.device)
    inst = np.array(starts, dtype=RENDER_INSTANCE_DTYPE)
    who = np.ascontiguousarray(subject_of, dtype=np.uint32).reshape(len(inst))
    inst["mesh"] = who
    host = np.ascontiguousarray(frames, dtype=np.uint16)
    d_frames = torch.from_numpy((host if host.flags.writeable else host.copy()).view(np.int16)).to(dev)
    d_who = torch.from_numpy(who.view(np.int32)).to(dev)
    d_inst = d_frec = d_urec = None
    for r in range(int(rounds)):
        d_inst, d_frec = fitter.fit(d_frames, subjects.models, inst, K_or_cameras, params=fit_prm, device_out=True, carried=d_inst)
        if r < int(shape_rounds):
            d_srec = fitter.shape_step_subjects(d_frames, subjects, d_inst, K_or_cameras, subjects=d_who, fit_records=d_frec, params=shape_prm,
                                                device_out=True)
            subjects.update(d_srec, device=True)
        d_urec = fitter.surface_step_subjects(d_frames, subjects, d_inst, K_or_cameras, subjects=d_who, fit_records=d_frec, params=surface_prm,
                                              device_out=True)
    torch.cuda.current_stream(dev).synchronize()
    if d_inst is None:
        return subjects.state(), inst, (np.zeros(len(inst), FIT_RECORD_DTYPE), np.zeros(len(subjects), SURFACE_RECORD_DTYPE))
    out = d_inst.cpu().numpy().view(RENDER_INSTANCE_DTYPE).copy()
    return subjects.state(), out, (d_frec.cpu().numpy().view(FIT_RECORD_DTYPE).copy(), d_urec.cpu().numpy().view(SURFACE_RECORD_DTYPE).copy())


def recognise_subjects(fitter, frames, K_or_cameras, subjects, starts, model, enrolled=None, fit_prm=None, ident_prm=None):
    """Say who each rough head of `frames` is, on the device.  frames [n, h, w] u16 (numpy) go to the device
    once; `starts` are RENDER_INSTANCE_DTYPE [m] rough poses.  Every start is fitted with `model` (the generic head: a `Model`)
    under fit_prm, then `Fitter.identify_subjects` runs from those poses and records against the candidates of `subjects` (a
    `Subjects` set; enrolled [S] marks them, None: all) under ident_prm -- all enqueued on the current torch stream, nothing read
    in between and once at the end.  Returns (subjects u32 [m] with IDENT_UNKNOWN for an unknown head, IDENT_RECORD_DTYPE [m], the
    instances at the best candidate's refitted pose, the generic fit's FIT_RECORD_DTYPE [m])."""
    import torch
    dev = torch.device("cuda", fitter.device)
    inst = np.array(starts, dtype=RENDER_INSTANCE_DTYPE)
    inst["mesh"] = 0
    if len(inst) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, IDENT_RECORD_DTYPE), inst, np.zeros(0, FIT_RECORD_DTYPE)
    host = np.ascontiguousarray(frames, dtype=np.uint16)
    d_frames = torch.from_numpy((host if host.flags.writeable else host.copy()).view(np.int16)).to(dev)
    d_enr = None
    if enrolled is not None:
        d_enr = torch.from_numpy(np.ascontiguousarray(np.asarray(enrolled) != 0, dtype=np.uint8).reshape(len(subjects))).to(dev)
    d_inst, d_frec = fitter.fit(d_frames, [model], inst, K_or_cameras, params=fit_prm, device_out=True)
    d_sub, d_rec, d_poses = fitter.identify_subjects(d_frames, subjects, d_inst, K_or_cameras, enrolled=d_enr, fit_records=d_frec, params=ident_prm,
                                                     device_out=True)
    torch.cuda.current_stream(dev).synchronize()
    return (d_sub.cpu().numpy().view(np.uint32).copy(), d_rec.cpu().numpy().view(IDENT_RECORD_DTYPE).copy(),
            d_poses.cpu().numpy().view(RENDER_INSTANCE_DTYPE).copy(), d_frec.cpu().numpy().view(FIT_RECORD_DTYPE).copy())


def recognise_subjects_views(fitter, frames, views, subjects, starts, model, enrolled=None, fit_prm=None, ident_prm=None):
    """`recognise_subjects` for one moment of a rig.  frames [n, h, w] u16 (numpy), camera c's frame at index
    c, go to the device once; `starts` are VIEW_INSTANCE_DTYPE [m] rough world poses with their view masks.  Every start is fitted
    with `model` (the generic head: a `Model`) over its views by `Fitter.fit_views` under fit_prm, then
    `Fitter.identify_subjects_views` runs from those instances and records with n_sets = 1 against the candidates of `subjects`
    under ident_prm -- all enqueued on the current torch stream, nothing read in between and once at the end.  Returns (subjects u32
    [m] with IDENT_UNKNOWN for an unknown head, IDENT_RECORD_DTYPE [m], the instances at the best candidate's refitted world pose,
    the generic fit's VIEW_FIT_RECORD_DTYPE [m])."""
    import torch
    dev = torch.device("cuda", fitter.device)
    inst = np.array(starts, dtype=VIEW_INSTANCE_DTYPE)
    inst["model"] = 0
    if len(inst) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, IDENT_RECORD_DTYPE), inst, np.zeros(0, VIEW_FIT_RECORD_DTYPE)
    host = np.ascontiguousarray(frames, dtype=np.uint16)
    d_frames = torch.from_numpy((host if host.flags.writeable else host.copy()).view(np.int16)).to(dev)
    d_enr = None
    if enrolled is not None:
        d_enr = torch.from_numpy(np.ascontiguousarray(np.asarray(enrolled) != 0, dtype=np.uint8).reshape(len(subjects))).to(dev)
    d_inst, d_frec = fitter.fit_views(d_frames, [model], inst, views, params=fit_prm, device_out=True)
    d_sub, d_rec, d_poses = fitter.identify_subjects_views(d_frames.reshape(1, *d_frames.shape), views, subjects, d_inst, enrolled=d_enr,
                                                           fit_records=d_frec, params=ident_prm, device_out=True)
    torch.cuda.current_stream(dev).synchronize()
    return (d_sub.cpu().numpy().view(np.uint32).copy(), d_rec.cpu().numpy().view(IDENT_RECORD_DTYPE).copy(),
            d_poses.cpu().numpy().view(VIEW_INSTANCE_DTYPE).copy(), d_frec.cpu().numpy().view(VIEW_FIT_RECORD_DTYPE).copy())


def adapt_views(fitter, frames, views, verts, tris, basis, starts, sets=None, rounds: int = 6, fit_prm=None, shape_prm=None, coeffs=None):
    """`adapt` over the views of a rig: frames [n_sets, n, h, w] u16 (numpy), `views` a `Views` of n
    cameras, `starts` VIEW_INSTANCE_DTYPE [m] world poses and sets [m] the set each belongs to (None: set 0).  A round builds
    the model from the current coefficients, fits every instance from its previous pose with Fitter.fit_views (one call per
    set, over the instances of that set), takes ONE multi-view shape step over the fits that ended FIT_OK and adds the
    increment when the step ended SHAPE_OK.  Returns what `adapt` returns: (coefficients [K] f64, the last fitted instances,
    trace); trace[r]["fit"] holds VIEW_FIT_RECORD_DTYPE records in the order of `starts`."""
    fields = np.ascontiguousarray(getattr(basis, "fields", basis), dtype=np.float32)
    c = np.zeros(len(fields), np.float64) if coeffs is None else np.array(coeffs, dtype=np.float64)
    inst = np.array(starts, dtype=VIEW_INSTANCE_DTYPE)
    st = np.zeros(len(inst), np.uint32) if sets is None else np.ascontiguousarray(sets, dtype=np.uint32).reshape(len(inst))
    trace = []
    with ShapeBasis(fields, device=fitter.device) as sb:
        for _ in range(int(rounds)):
            v = deform(verts, fields, c)
            with Model(v, vertex_normals(v, tris), device=fitter.device) as model:
                rec = np.zeros(len(inst), VIEW_FIT_RECORD_DTYPE)
                for s in np.unique(st):
                    of = np.flatnonzero(st == s)
                    one = inst[of].copy()
                    one["model"] = 0
                    out, rec[of] = fitter.fit_views(frames[int(s)], [model], one, views, params=fit_prm)
                    inst["R"][of], inst["t"][of] = out["R"], out["t"]
                subj = np.where(rec["status"] == FIT_OK, 0, SHAPE_SKIP).astype(np.uint32)
                srec = fitter.shape_step_views(frames, views, model, sb, inst, sets=st, subjects=subj, params=shape_prm)[0]
            delta = srec["delta"][:len(c)].copy() if srec["status"] == SHAPE_OK else np.zeros(len(c))
            trace.append({"coeffs": c.copy(), "fit": rec, "shape": srec, "delta": delta})
            c = c + delta
    return c, inst, trace


def calibrate_views(fitter, frames, cameras, V, u, model, starts, sets=None, hold=None, steps: int = 8, wide_steps: int = 3,
                    gates=(60.0, 25.0), rounds: int = 3, joint_steps: int = 2, fit_prm=None, refit_prm=None, lam=None, min_points=None):
    """Calibrate the extrinsics (V [n, 3, 3], u [n, 3]) of the cameras of `cameras` from frames [n_sets, n, h, w] u16 (numpy) of
    one head model moved through the volume.  `starts` are VIEW_INSTANCE_DTYPE [m] rough world poses
    whose `views` name every camera that sees the instance, sets [m] the set of each (None: set 0), hold [n] marks the gauge
    cameras, whose entries are trusted and stay as they are: at least one is needed.  Three stages:
      1. every instance is fitted against the HELD cameras among its views only (fit_prm);
      2. `steps` calibration steps with the pivot at the mean fitted position, the first `wide_steps` at gates[0], the others
         at gates[1], over the fits that ended FIT_OK, a new table after each;
      3. `rounds` times: every instance is refitted against ALL its views from its last pose (refit_prm, default no coarse and
         6 full steps), then `joint_steps` calibration steps at gates[1].
    Each step waits on the host: this happens once per rig, not once per frame.  Returns (V, u, the last instances, trace):
    trace is a list of {"stage", "records" (CALIB_RECORD_DTYPE [n]), "fit" (the VIEW_FIT_RECORD_DTYPE [m] records the step's
    poses came from)}."""
    V = np.array(V, dtype=np.float32).reshape(-1, 3, 3)
    u = np.array(u, dtype=np.float32).reshape(-1, 3)
    n = len(V)
    inst = np.array(starts, dtype=VIEW_INSTANCE_DTYPE)
    st = np.zeros(len(inst), np.uint32) if sets is None else np.ascontiguousarray(sets, dtype=np.uint32).reshape(len(inst))
    hd = np.zeros(n, np.uint8) if hold is None else (np.asarray(hold).reshape(n) != 0).astype(np.uint8)
    if refit_prm is None:
        refit_prm = fit_params(coarse_iterations=0, iterations=6)
    all_views = inst["views"].copy()
    held_mask = np.zeros(len(inst), np.uint64)
    for i, s in enumerate(inst):
        m = 0
        for k in range(64):
            c = int(s["first_cam"]) + k
            if (int(s["views"]) >> k) & 1 and c < n and hd[c]:
                m |= 1 << k
        held_mask[i] = m
    trace = []

    def fit_all(table, masks, prm):
        rec = np.zeros(len(inst), VIEW_FIT_RECORD_DTYPE)
        rec["status"] = FIT_FEW_POINTS
        for s in np.unique(st):
            of = np.flatnonzero((st == s) & (masks != 0))
            if not len(of):
                continue
            one = inst[of].copy()
            one["model"], one["views"] = 0, masks[of]
            out, rec[of] = fitter.fit_views(frames[int(s)], [model], one, table, params=prm)
            inst["R"][of], inst["t"][of] = out["R"], out["t"]
        return rec

    def calib(table, rec, gate, stage):
        nonlocal V, u
        ok = rec["status"] == FIT_OK
        pivot = inst["t"][ok].astype(np.float64).mean(axis=0) if ok.any() else np.zeros(3)
        take = np.where(ok, 0, CALIB_SKIP).astype(np.uint32)
        crec = fitter.calibrate_step(frames, table, model, inst, sets=st, take=take, hold=hd,
                                     params=calib_params(gate=gate, lam=lam, min_points=min_points, pivot=pivot))
        trace.append({"stage": stage, "records": crec, "fit": rec})
        nxt = views_from_records(cameras, V, u, crec)
        V, u = nxt.V, nxt.u
        table.close()
        return nxt

    table = Views(cameras, V, u)
    try:
        rec = fit_all(table, held_mask, fit_prm)
        inst["views"] = all_views
        for k in range(int(steps)):
            table = calib(table, rec, gates[0] if k < int(wide_steps) else gates[1], "held")
        for r in range(int(rounds)):
            rec = fit_all(table, all_views, refit_prm)
            for _ in range(int(joint_steps)):
                table = calib(table, rec, gates[1], f"joint {r}")
    finally:
        table.close()
    return V, u, inst, trace


def fit_track_params(iterations_tracked=None, keep_points=None, rms_max=None, max_jump=None, conf=None, min_windows=None,
                     max_coast=None) -> "_lib.FitTrackParams":
    """dh_fit_track_params_default with the given fields replaced; `conf` is (conf_num, conf_den)."""
    p = _params(_lib.FitTrackParams, "dh_fit_track_params_default", iterations_tracked=iterations_tracked, keep_points=keep_points, rms_max=rms_max,
                max_jump=max_jump, min_windows=min_windows, max_coast=max_coast)
    if conf is not None:
        p.conf_num, p.conf_den = int(conf[0]), int(conf[1])
    return p


def angles() -> np.ndarray:
    """The tracker's angle table [120, 2] f64: (cos, sin) of (i - 60) / 60 * 3.14159 as the library computed them."""
    out = np.zeros((FIT_TRACK_ANGLES, 2), np.float64)
    check(_lib.load().dh_fit_tracker_angles(vp(out)))
    return out


def rig_fit_track_params(iterations_tracked=None, keep_points=None, rms_max=None, max_jump=None, max_coast=None,
                         max_misses=None) -> "_lib.RigFitTrackParams":
    """dh_rig_fit_track_params_default with the given fields replaced; `max_misses` is the rig tracker's, which the ids come from."""
    return _params(_lib.RigFitTrackParams, "dh_rig_fit_track_params_default", iterations_tracked=iterations_tracked, keep_points=keep_points,
                   rms_max=rms_max, max_jump=max_jump, max_coast=max_coast, max_misses=max_misses)


def subject_track_params(retry=None, max_tries=None) -> "_lib.SubjectTrackParams":
    """dh_subject_track_params_default with the given fields replaced."""
    return _params(_lib.SubjectTrackParams, "dh_subject_track_params_default", retry=retry, max_tries=max_tries)


class _FitTrackerBase(_lib._Handle):
    """What the four fit trackers share: the handle, self.n cameras of self.h x self.w, and what a host step
    makes of its frames and present bytes.  A class sets _prefix, the C name its entry points begin with, and the dtypes of its
    records and of its state."""
    _prefix = _record_dtype = _state_dtype = None

    def _open(self, model: Model, w: int, h: int, motion: bool, n: int) -> None:
        self._lib = _lib.load()
        self.model, self.w, self.h, self.n = model, int(w), int(h), n
        self.flags = FIT_TRACK_MOTION if motion else 0
        self._h = C.c_void_p()

    def _call(self, name: str, *args) -> None:
        check(getattr(self._lib, f"{self._prefix}_{name}")(*args))

    def _frames(self, frames) -> np.ndarray:
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        if frames.shape != (self.n, self.h, self.w):
            raise ValueError(f"frames must be [{self.n}, {self.h}, {self.w}]")
        return frames

    def _present(self, present):
        return None if present is None else np.ascontiguousarray(present, dtype=np.uint8).reshape(self.n)

    def _reset(self, unit, stream) -> None:
        self._call("reset", self._h, C.c_int(-1 if unit is None else int(unit)), C.c_void_p(int(stream)))

    def _state(self, *shape) -> np.ndarray:
        st = np.zeros(shape, self._state_dtype)
        self._call("state", self._h, vp(st))
        return st


class _SubjectBound:
    """What a binding to a `Subjects` set (self.subjects, S subjects) adds to a fit tracker; `bind` is the tracker's own."""

    def _mask(self, enrolled):
        return None if enrolled is None else np.ascontiguousarray(enrolled, dtype=np.uint8).reshape(len(self.subjects))

    def info(self):
        """(cameras of a SubjectFitTracker, rigs of a RigSubjectFitTracker; S; the workgroups of the score kernel's grid), ints."""
        n, s, g = C.c_int(), C.c_uint32(), C.c_uint32()
        self._call("info", self._h, C.byref(n), C.byref(s), C.byref(g))
        return n.value, s.value, g.value

    def set_enrolled(self, enrolled, stream: int = 0) -> None:
        """Replace the candidates' mask (u8 [S], None: all); stream-ordered."""
        self._call("set_enrolled", self._h, vp(self._mask(enrolled)), C.c_void_p(int(stream)))


class _CameraFitTracker(_FitTrackerBase):
    """The steps of the camera pair.  Records: FIT_TRACK_RECORD_DTYPE [n] of a FitTracker, SUBJECT_TRACK_RECORD_DTYPE [n] of a
    SubjectFitTracker (dh_fit_track_record, dh_subject_track_record on the device)."""

    def step_poses(self, frames, poses, support, present=None, fit_params=None) -> np.ndarray:
        """The core step from the forest's POSE_DTYPE [n] and SUPPORT_DTYPE [n] of host frames [n, h, w] u16 (present: u8 [n] or
        None): -> the records [n], FIT_TRACK_RECORD_DTYPE or SUBJECT_TRACK_RECORD_DTYPE."""
        frames, pr = self._frames(frames), self._present(present)
        poses = np.ascontiguousarray(poses, dtype=POSE_DTYPE).reshape(self.n)
        support = np.ascontiguousarray(support, dtype=SUPPORT_DTYPE).reshape(self.n)
        rec = np.zeros(self.n, self._record_dtype)
        self._call("step_poses", self._h, vp(frames), self.w, self.h, vp(pr), vp(poses), vp(support), _lib.ref(fit_params), vp(rec))
        return rec

    def step(self, hp, frames, present=None, radius: int = SUPPORT_RADIUS, fit_params=None):
        """The whole step: `hp` (a HoughPrediction) predicts every camera's pose and support without guesses, then the core
        step, on one stream.  -> (POSE_DTYPE [n], SUPPORT_DTYPE [n], the records [n], FIT_TRACK_RECORD_DTYPE or
        SUBJECT_TRACK_RECORD_DTYPE)."""
        frames, pr = self._frames(frames), self._present(present)
        poses, support = np.zeros(self.n, POSE_DTYPE), np.zeros(self.n, SUPPORT_DTYPE)
        rec = np.zeros(self.n, self._record_dtype)
        self._call("step", hp._ph, self._h, vp(frames), self.w, self.h, vp(pr), C.c_uint32(int(radius) & 0xFFFFFFFF),
                   _lib.ref(fit_params), vp(poses), vp(support), vp(rec))
        return poses, support, rec

    def step_device(self, frames_ptr: int, poses_ptr: int, support_ptr: int, records_ptr: int, hp=None, present_ptr: int = 0,
                    radius: int = SUPPORT_RADIUS, fit_params=None, stream: int = 0) -> None:
        """Device frames [n][h][w] u16, poses [n] dh_pose, support [n] dh_support, records [n] dh_fit_track_record (of a
        SubjectFitTracker: dh_subject_track_record), present [n] u8 or 0.  With `hp` the whole step (poses and support are
        outputs), without it the core step (they are inputs).  Asynchronous on `stream`: three launches (of a SubjectFitTracker:
        five) after the prediction's; allocates nothing and never waits on the host."""
        prm, present, stream = _lib.ref(fit_params), vp(present_ptr or None), C.c_void_p(int(stream))
        if hp is None:
            self._call("step_poses_device", self._h, vp(frames_ptr), self.w, self.h, present, vp(poses_ptr), vp(support_ptr), prm,
                       vp(records_ptr), stream)
        else:
            self._call("step_device", hp._ph, self._h, vp(frames_ptr), self.w, self.h, present, C.c_uint32(int(radius) & 0xFFFFFFFF), prm,
                       vp(poses_ptr), vp(support_ptr), vp(records_ptr), stream)

    def reset(self, camera: int | None = None, stream: int = 0) -> None:
        """One camera or all back to the initial state (nothing tracked, and of a SubjectFitTracker nobody bound); stream-ordered."""
        self._reset(camera, stream)

    def state(self) -> np.ndarray:
        """Synchronous copy of the state: FIT_TRACK_STATE_DTYPE [n], of a SubjectFitTracker SUBJECT_TRACK_STATE_DTYPE [n]."""
        return self._state(self.n)


class FitTracker(_CameraFitTracker):
    """One dh_fit_tracker: each camera of `cameras` (a `tracking.Cameras`) carries its fitted head pose from
    step to step.  A step fits `model` to every present camera's frame -- from the carried pose, or from the forest's where
    there is none -- and decides whether the fit is believed; a rejected fit sends the camera back to the forest.  The state
    stays on the device.  Steps of one tracker must be stream-ordered; the camera table and the model must outlive it."""
    _handles = (("_h", "dh_fit_tracker_destroy"),)
    _prefix, _record_dtype, _state_dtype = "dh_fit_tracker", FIT_TRACK_RECORD_DTYPE, FIT_TRACK_STATE_DTYPE

    def __init__(self, cameras, model: Model, w: int, h: int, scale: float = 1.0, motion: bool = False, params=None):
        self._open(model, w, h, motion, len(cameras))
        self.cameras = cameras
        self._call("create", cameras._h, model._h, C.c_float(scale), C.c_uint32(self.flags), _lib.ref(params), C.byref(self._h))

    @staticmethod
    def angles() -> np.ndarray:
        return angles()


class SubjectFitTracker(_SubjectBound, _CameraFitTracker):
    """One dh_subject_fit_tracker: a `FitTracker` bound to a `Subjects` set.  A track that starts is
    followed with `model` (the generic head), identified against the set's enrolled subjects on the device, and from the next
    step on followed with its own subject's model as the set holds it.  `enrolled` [S] (None: all) says which subjects are
    candidates.  The state stays on the device; a step never waits on the host.  Steps, resets, binds and mask changes of one
    tracker must be stream-ordered with one another and with the set's updates; the camera table, the set and the model must
    outlive it."""
    _handles = (("_h", "dh_subject_fit_tracker_destroy"),)
    _prefix, _record_dtype, _state_dtype = "dh_subject_fit_tracker", _lib.SUBJECT_TRACK_RECORD_DTYPE, _lib.SUBJECT_TRACK_STATE_DTYPE

    def __init__(self, cameras, subjects: Subjects, model: Model, w: int, h: int, scale: float = 1.0, motion: bool = False, params=None,
                 ident_params=None, subject_params=None, enrolled=None):
        self._open(model, w, h, motion, len(cameras))
        self.cameras, self.subjects = cameras, subjects
        self._call("create", cameras._h, subjects._h, model._h, C.c_float(scale), C.c_uint32(self.flags), _lib.ref(params),
                   _lib.ref(ident_params), _lib.ref(subject_params), vp(self._mask(enrolled)), C.byref(self._h))

    def bind(self, camera: int, subject: int | None, stream: int = 0) -> None:
        """The caller's own binding of `camera` to `subject`; None unbinds.  Stream-ordered."""
        self._call("bind", self._h, C.c_int(int(camera)), C.c_uint32(IDENT_UNKNOWN if subject is None else int(subject)),
                   C.c_void_p(int(stream)))


class _RigFitTracker(_FitTrackerBase):
    """The steps of the rig pair over self.n_rigs rigs of self.n cameras in all.  Records: RIG_FIT_RECORD_DTYPE [n_rigs,
    RIG_MAX_TRACKS] of a RigFitTracker, RIG_SUBJECT_RECORD_DTYPE [n_rigs, RIG_MAX_TRACKS] of a RigSubjectFitTracker
    (dh_rig_fit_record, dh_rig_subject_record on the device)."""

    def _open_rig(self, rig, views: Views, model: Model, w: int, h: int, motion: bool) -> None:
        self._open(model, w, h, motion, rig.n)
        self.rig, self.views, self.n_rigs = rig, views, rig.n_rigs

    def _records(self) -> np.ndarray:
        return np.zeros((self.n_rigs, RIG_MAX_TRACKS), self._record_dtype)

    def step_persons(self, frames, n_heads, heads, n_persons, persons, present=None, fit_params=None) -> np.ndarray:
        """The core step from the outputs of a rig tracker step -- n_heads u32 [n_cams], HEAD_DTYPE [n_cams, max_heads], n_persons
        u32 [n_rigs], RIG_PERSON_DTYPE [n_rigs, RIG_MAX_PERSONS] -- and host frames [n_cams, h, w] u16 (present: u8 [n_cams] or
        None): -> the records [n_rigs, RIG_MAX_TRACKS], RIG_FIT_RECORD_DTYPE or RIG_SUBJECT_RECORD_DTYPE."""
        frames, pr = self._frames(frames), self._present(present)
        heads = np.ascontiguousarray(heads, dtype=HEAD_DTYPE)
        if heads.ndim != 2 or heads.shape[0] != self.n:
            raise ValueError(f"heads must be [{self.n}, max_heads]")
        n_heads = np.ascontiguousarray(n_heads, dtype=np.uint32).reshape(self.n)
        n_persons = np.ascontiguousarray(n_persons, dtype=np.uint32).reshape(self.n_rigs)
        persons = np.ascontiguousarray(persons, dtype=RIG_PERSON_DTYPE).reshape(self.n_rigs, RIG_MAX_PERSONS)
        rec = self._records()
        self._call("step_persons", self._h, vp(frames), self.w, self.h, vp(pr), C.c_int(heads.shape[1]), vp(n_heads), vp(heads),
                   vp(n_persons), vp(persons), _lib.ref(fit_params), vp(rec))
        return rec

    def step(self, rig_tracker, frames, present=None, tracks: bool = True, fit_params=None):
        """The whole step: `rig_tracker` (a `tracking.RigTracker` of the same rig table) steps on the frames, then the core
        step, on one stream.  -> (what RigTracker.step returns: n_heads, heads, rig_ids, n_persons, persons, tracks or None;
        the records [n_rigs, RIG_MAX_TRACKS], RIG_FIT_RECORD_DTYPE or RIG_SUBJECT_RECORD_DTYPE)."""
        frames, pr = self._frames(frames), self._present(present)
        mh = rig_tracker.max_heads
        n_heads, heads = np.zeros(self.n, np.uint32), np.zeros((self.n, mh), HEAD_DTYPE)
        ids = np.zeros((self.n, mh), np.uint32)
        n_persons, persons = np.zeros(self.n_rigs, np.uint32), np.zeros((self.n_rigs, RIG_MAX_PERSONS), RIG_PERSON_DTYPE)
        tr = np.zeros((self.n_rigs, RIG_MAX_TRACKS), RIG_TRACK_DTYPE) if tracks else None
        rec = self._records()
        self._call("step", rig_tracker.hp._ph, self._h, rig_tracker._h, vp(frames), self.w, self.h, vp(pr), _lib.ref(fit_params),
                   vp(n_heads), vp(heads), vp(ids), vp(n_persons), vp(persons), vp(tr), vp(rec))
        return (n_heads, heads, ids, n_persons, persons, tr), rec

    def step_device(self, frames_ptr: int, n_heads_ptr: int, heads_ptr: int, n_persons_ptr: int, persons_ptr: int, records_ptr: int,
                    max_heads: int = MAX_HEADS, rig_tracker=None, ids_ptr: int = 0, tracks_ptr: int = 0, present_ptr: int = 0,
                    fit_params=None, stream: int = 0) -> None:
        """Device frames [n_cams][h][w] u16, n_heads [n_cams] u32, heads [n_cams][max_heads] dh_head, n_persons [n_rigs] u32,
        persons [n_rigs][RIG_MAX_PERSONS] dh_rig_person, records [n_rigs][RIG_MAX_TRACKS] dh_rig_fit_record (of a
        RigSubjectFitTracker: dh_rig_subject_record), present [n_cams] u8 or 0.  With `rig_tracker` the whole step (heads and
        persons are outputs, as are rig_ids [n_cams][max_heads] u32 and, unless 0, tracks; max_heads is the rig tracker's),
        without it the core step (they are inputs).  Asynchronous on `stream`: three launches (of a RigSubjectFitTracker: five)
        after the rig tracker's; allocates nothing and never waits on the host."""
        prm, present, stream = _lib.ref(fit_params), vp(present_ptr or None), C.c_void_p(int(stream))
        if rig_tracker is None:
            self._call("step_persons_device", self._h, vp(frames_ptr), self.w, self.h, present, C.c_int(int(max_heads)), vp(n_heads_ptr),
                       vp(heads_ptr), vp(n_persons_ptr), vp(persons_ptr), prm, vp(records_ptr), stream)
        else:
            self._call("step_device", rig_tracker.hp._ph, self._h, rig_tracker._h, vp(frames_ptr), self.w, self.h, present, prm,
                       vp(n_heads_ptr), vp(heads_ptr), vp(ids_ptr or None), vp(n_persons_ptr), vp(persons_ptr), vp(tracks_ptr or None),
                       vp(records_ptr), stream)

    def reset(self, rig: int | None = None, stream: int = 0) -> None:
        """One rig or all back to the initial state (every entry free, and of a RigSubjectFitTracker nobody bound); stream-ordered."""
        self._reset(rig, stream)

    def state(self) -> np.ndarray:
        """Synchronous copy of the state: RIG_FIT_STATE_DTYPE [n_rigs, RIG_MAX_TRACKS], of a RigSubjectFitTracker
        RIG_SUBJECT_STATE_DTYPE [n_rigs, RIG_MAX_TRACKS]."""
        return self._state(self.n_rigs, RIG_MAX_TRACKS)


class RigFitTracker(_RigFitTracker):
    """One dh_rig_fit_tracker: every person of every rig of `rig` (a `tracking.Rig`) keeps one fitted pose in
    the world frame under the id a `tracking.RigTracker` gave it.  A step refits `model` against all the views (`views`, a `Views`
    of the rig's camera table, consistent with the rig: `views_from_rig`) from the carried pose, or from the person record where
    there is none, and decides whether the fit is believed.  The state stays on the device.  Steps of one tracker must be
    stream-ordered; the tables and the model must outlive it."""
    _handles = (("_h", "dh_rig_fit_tracker_destroy"),)
    _prefix, _record_dtype, _state_dtype = "dh_rig_fit_tracker", RIG_FIT_RECORD_DTYPE, RIG_FIT_STATE_DTYPE

    def __init__(self, rig, views: Views, model: Model, w: int, h: int, scale: float = 1.0, motion: bool = False, params=None):
        self._open_rig(rig, views, model, w, h, motion)
        self._call("create", rig._h, views._h, model._h, C.c_float(scale), C.c_uint32(self.flags), _lib.ref(params), C.byref(self._h))


class RigSubjectFitTracker(_SubjectBound, _RigFitTracker):
    """One dh_rig_subject_fit_tracker: a `RigFitTracker` bound to a `Subjects` set.  An entry that starts is
    followed with `model` (the generic head), identified over all its present views against the set's enrolled subjects on the
    device, and from the next step on fitted with its own subject's model as the set holds it.  `enrolled` [S] (None: all) says
    which subjects are candidates.  The state stays on the device; a step never waits on the host.  Steps, resets, binds and mask
    changes of one tracker must be stream-ordered with one another and with the set's updates; the tables, the set and the model
    must outlive it."""
    _handles = (("_h", "dh_rig_subject_fit_tracker_destroy"),)
    _prefix, _record_dtype, _state_dtype = "dh_rig_subject_fit_tracker", _lib.RIG_SUBJECT_RECORD_DTYPE, _lib.RIG_SUBJECT_STATE_DTYPE

    def __init__(self, rig, views: Views, subjects: Subjects, model: Model, w: int, h: int, scale: float = 1.0, motion: bool = False,
                 params=None, ident_params=None, subject_params=None, enrolled=None):
        self._open_rig(rig, views, model, w, h, motion)
        self.subjects = subjects
        self._call("create", rig._h, views._h, subjects._h, model._h, C.c_float(scale), C.c_uint32(self.flags), _lib.ref(params),
                   _lib.ref(ident_params), _lib.ref(subject_params), vp(self._mask(enrolled)), C.byref(self._h))

    def bind(self, rig: int, rig_id: int, subject: int | None, stream: int = 0) -> None:
        """The caller's own binding of the entry of `rig` that holds `rig_id` to `subject`; None unbinds; an id nobody holds changes
        nothing.  Stream-ordered."""
        self._call("bind", self._h, C.c_int(int(rig)), C.c_uint32(int(rig_id)), C.c_uint32(IDENT_UNKNOWN if subject is None else int(subject)),
                   C.c_void_p(int(stream)))
