"""Posed triangle meshes rendered to depth frames and head masks on the GPU: what a Kinect would have
recorded of a head mesh at a pose, left on the device for training, prediction, tracking and rigs.  All arithmetic runs in
libdepthhead_hip.so (k_render.hip); the rule is stated in include/depthhead_hip.h."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import RENDER_HEAD, RENDER_INSTANCE_DTYPE, check, vp


def euler_to_matrix(rot_deg) -> np.ndarray:
    """The rotation matrix (3 x 3 f32) of three pose angles in DEGREES, in the camera frame (x right, y down, z forward).

    PARITY UNPINNED: the reference never turns the three angles into a matrix on its prediction path.  Its viewer draws the
    head model turned by rotx(-rot[2]) * roty(-rot[1]) * rotz(rot[0]) (utils/src/headwin.rs:82-84 with the column-major arrays
    of :150-170, applied in that order to the vertex at :285), which in the usual row convention is
    V = Rx(-rot[2]) Ry(rot[1]) Rz(rot[0]); its frame is the camera frame with y negated, so the camera-frame matrix is F V F with
    F = diag(1, -1, 1) = Rx(rot[2]) Ry(rot[1]) Rz(-rot[0]).  The same convention as tracking.world_rotation, which takes radians.
    Computed in f64 on the host and rounded to f32 once."""
    r0, r1, r2 = (float(v) for v in np.radians(np.asarray(rot_deg, dtype=np.float64).reshape(3)))
    c, s = np.cos, np.sin
    rx = np.array([[1, 0, 0], [0, c(r2), -s(r2)], [0, s(r2), c(r2)]])
    ry = np.array([[c(r1), 0, s(r1)], [0, 1, 0], [-s(r1), 0, c(r1)]])
    rz = np.array([[c(-r0), -s(-r0), 0], [s(-r0), c(-r0), 0], [0, 0, 1]])
    return (rx @ ry @ rz).astype(np.float32)


def parse_obj(text: str):
    """(verts [nv, 3] f32, tris [nt, 3] u32) of Wavefront OBJ text: `v` and `f` lines only, polygons fan-triangulated, negative
    indices counted back from the vertices read so far, `/vt/vn` suffixes ignored."""
    verts, tris = [], []
    for line in text.splitlines():
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        if tok[0] == "v":
            if len(tok) < 4:
                raise ValueError(f"OBJ vertex with fewer than three coordinates: {line!r}")
            verts.append([float(tok[1]), float(tok[2]), float(tok[3])])
        elif tok[0] == "f":
            idx = []
            for item in tok[1:]:
                i = int(item.split("/", 1)[0])
                i = i - 1 if i > 0 else len(verts) + i
                if i < 0 or i >= len(verts) or item.startswith("0"):
                    raise ValueError(f"OBJ face index out of range: {line!r}")
                idx.append(i)
            if len(idx) < 3:
                raise ValueError(f"OBJ face with fewer than three vertices: {line!r}")
            for k in range(1, len(idx) - 1):
                tris.append([idx[0], idx[k], idx[k + 1]])
    return np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(tris, dtype=np.uint32).reshape(-1, 3)


class Mesh(_lib._Handle):
    """One dh_mesh: vertices [nv, 3] (mm) and triangles [nt, 3] on `device`; the host copies stay in `verts` / `tris`."""
    _handles = (("_h", "dh_mesh_destroy"),)

    def __init__(self, verts, tris, device: int = 0):
        self._lib = _lib.load()
        self.verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        t = np.asarray(tris)
        if t.size and (t.min() < 0 or t.max() > 0xFFFFFFFF):
            raise ValueError("triangle index outside 0 .. 2^32 - 1")
        self.tris = np.ascontiguousarray(t, dtype=np.uint32).reshape(-1, 3)
        self.device = int(device)
        self._h = C.c_void_p()
        check(self._lib.dh_mesh_create(vp(self.verts), C.c_uint32(len(self.verts)), vp(self.tris), C.c_uint32(len(self.tris)),
                                       self.device, C.byref(self._h)))

    @classmethod
    def from_obj(cls, path_or_text, device: int = 0) -> "Mesh":
        s = os.fspath(path_or_text)
        if "\n" not in s and os.path.exists(s):
            with open(s) as f:
                s = f.read()
        return cls(*parse_obj(s), device=device)

    def info(self):
        """(nv, nt, bbox[6] = min x, y, z, max x, y, z) as the library holds them."""
        nv, nt = C.c_uint32(), C.c_uint32()
        bbox = np.zeros(6, np.float32)
        check(self._lib.dh_mesh_info(self._h, C.byref(nv), C.byref(nt), vp(bbox)))
        return nv.value, nt.value, bbox

    def bounding_radius(self) -> float:
        """Largest distance of a vertex from the mesh's origin."""
        return float(np.sqrt((self.verts.astype(np.float64) ** 2).sum(axis=1).max()))


def instances(items) -> np.ndarray:
    """A dh_render_instance array from (frame, mesh, R [3, 3], t [3], scale, head) tuples."""
    out = np.zeros(len(items), dtype=RENDER_INSTANCE_DTYPE)
    for i, (frame, mesh, R, t, scale, head) in enumerate(items):
        out[i] = (frame, mesh, np.asarray(R, dtype=np.float32).reshape(9), np.asarray(t, dtype=np.float32).reshape(3), scale,
                  RENDER_HEAD if head else 0)
    return out


class Renderer(_lib._Handle):
    """One dh_renderer on `device`.  Not thread-safe."""
    _handles = (("_h", "dh_renderer_destroy"),)

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        self.device = int(device)
        self._h = C.c_void_p()
        check(self._lib.dh_renderer_create(self.device, C.byref(self._h)))

    def render(self, meshes, instances, n, w, h, K_or_cameras, noise: int = 0, holes: float = 0.0, seed: int = 0,
               device_out: bool = False, masks: bool = True, stream=None):
        """Draw `instances` (a RENDER_INSTANCE_DTYPE array, see `instances()`) of `meshes` into n frames of w x h seen through
        one K ([3, 3] or an `IntrinsicMatrix`) or a `tracking.Cameras` table of exactly n cameras.  Returns (frames [n, h, w] u16, masks [n, h, w] u8) as numpy
        arrays, or as torch tensors on the device with device_out=True (ordered on `stream`, default the current torch
        stream); masks=False skips the mask (None is returned for it)."""
        inst = np.ascontiguousarray(instances, dtype=RENDER_INSTANCE_DTYPE)
        meshes = list(meshes)
        handles = (C.c_void_p * max(len(meshes), 1))(*[m._h.value for m in meshes])
        prm = _lib.RenderParams(int(noise), 0, float(holes), int(seed) & 0xFFFFFFFFFFFFFFFF, (C.c_uint64 * 2)(0, 0))
        kind, karg = _lib.intrinsics(K_or_cameras)
        n, w, h = int(n), int(w), int(h)
        head = (self._h, handles, C.c_uint32(len(meshes)), vp(inst) if len(inst) else None, C.c_uint32(len(inst)), n, w, h, karg,
                C.byref(prm))
        if not device_out:
            shape = (max(n, 0), max(h, 0), max(w, 0))
            frames = np.zeros(shape, np.uint16)
            mk = np.zeros(shape, np.uint8) if masks else None
            check(getattr(self._lib, "dh_render_depth" + kind)(*head, vp(frames), vp(mk)))
            return frames, mk
        import torch
        dev = torch.device("cuda", self.device)
        shape = (max(n, 0), max(h, 0), max(w, 0))
        frames = torch.empty(shape, dtype=torch.int16, device=dev)      # (the bits are u16: viewed as such where torch has the type)
        if hasattr(torch, "uint16"):
            frames = frames.view(torch.uint16)
        mk = torch.empty(shape, dtype=torch.uint8, device=dev) if masks else None
        check(getattr(self._lib, "dh_render_depth" + kind + "_device")(*head, C.c_void_p(frames.data_ptr()),
                                                                         C.c_void_p(mk.data_ptr()) if masks else None,
                                                                         C.c_void_p(_lib.stream_of(self.device, stream))))
        return frames, mk

    def set_profiling(self, on: bool) -> None:
        check(self._lib.dh_renderer_set_profiling(self._h, int(bool(on))))

    def timing(self) -> dict:
        """Device time in ms of the last profiled render's kernels."""
        ms = (C.c_float * 4)()
        check(self._lib.dh_renderer_timing(self._h, ms))
        return dict(zip(("setup_ms", "offsets_ms", "fill_ms", "resolve_ms"), (float(v) for v in ms)))
