"""The render entry points without a GPU: exported and declared, the dh_render_instance / dh_render_params layouts of the Python
side equal the C layout (a g++ program prints sizeof and offsetof from include/depthhead_hip.h), and every refusal answers
DH_EINVAL with a message and leaves the output buffers untouched."""
import ctypes as C

import numpy as np

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib

NEW = ["dh_mesh_create", "dh_mesh_destroy", "dh_mesh_info", "dh_renderer_create", "dh_renderer_destroy", "dh_renderer_set_profiling",
       "dh_renderer_timing", "dh_render_depth", "dh_render_depth_cameras", "dh_render_depth_device", "dh_render_depth_cameras_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_render_instance size %zu\n", sizeof(dh_render_instance));
    F(dh_render_instance, frame); F(dh_render_instance, mesh); F(dh_render_instance, R); F(dh_render_instance, t);
    F(dh_render_instance, scale); F(dh_render_instance, flags);
    printf("dh_render_params size %zu\n", sizeof(dh_render_params));
    F(dh_render_params, noise_amplitude); F(dh_render_params, reserved0); F(dh_render_params, hole_probability);
    F(dh_render_params, seed); F(dh_render_params, reserved);
    printf("consts %d %d %d\n", (int)DH_RENDER_HEAD, DH_RENDER_MAX_SIZE, DH_VERSION);
    return 0;
}
"""


def test_render_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    import depthhead_amd
    from depthhead_amd import render, synth, training
    for name in ("Mesh", "Renderer", "euler_to_matrix"):
        assert hasattr(depthhead_amd, name) and name in depthhead_amd.__all__, name
    assert callable(render.Mesh.from_obj) and callable(render.Renderer.render)
    assert callable(synth.head_mesh) and callable(training.rendered_data)


def test_header_declares_every_render_export():
    abi_kit.assert_header_equals_exports(NEW, "#define DH_VERSION 100")


def test_layouts_match_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    consts = [int(v) for v in consts]
    assert consts == [_lib.RENDER_HEAD, _lib.RENDER_MAX_SIZE, 100] == [1, 16384, 100]
    dt = _lib.RENDER_INSTANCE_DTYPE
    assert c[("dh_render_instance", "size")] == dt.itemsize == 64
    for f in dt.names:
        assert c[("dh_render_instance", f)] == dt.fields[f][1], f
    assert sum(dt.fields[f][0].itemsize for f in dt.names) == dt.itemsize          # no padding
    assert c[("dh_render_params", "size")] == C.sizeof(_lib.RenderParams) == 40
    for f, _ in _lib.RenderParams._fields_:
        assert c[("dh_render_params", f)] == getattr(_lib.RenderParams, f).offset, f


def test_mesh_create_refusals(hip_lib):
    lib, vp = hip_lib, _lib.vp
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    t = np.array([[0, 1, 2]], np.uint32)
    h = C.c_void_p(1234)
    assert lib.dh_mesh_create(None, 3, vp(t), 1, 0, C.byref(h)) == EINVAL and "NULL" in _err(lib) and h.value is None
    assert lib.dh_mesh_create(vp(v), 3, None, 1, 0, C.byref(h)) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_mesh_create(vp(v), 3, vp(t), 1, 0, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_mesh_create(vp(v), 0, vp(t), 1, 0, C.byref(h)) == EINVAL and "at least one" in _err(lib)
    assert lib.dh_mesh_create(vp(v), 3, vp(t), 0, 0, C.byref(h)) == EINVAL and "at least one" in _err(lib)
    bad = np.array([[0, 1, 3]], np.uint32)
    assert lib.dh_mesh_create(vp(v), 3, vp(bad), 1, 0, C.byref(h)) == EINVAL and "names vertex 3 of 3" in _err(lib)
    for x in (np.nan, np.inf, -np.inf):
        w = v.copy(); w[2, 1] = x
        assert lib.dh_mesh_create(vp(w), 3, vp(t), 1, 0, C.byref(h)) == EINVAL and "vertex 2 is not finite" in _err(lib)
    assert h.value is None
    assert lib.dh_mesh_destroy(None) == 0 and lib.dh_renderer_destroy(None) == 0
    assert lib.dh_mesh_info(None, None, None, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_renderer_create(0, None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_renderer_set_profiling(None, 1) == EINVAL and lib.dh_renderer_timing(None, None) == EINVAL


def test_render_refusals_leave_the_outputs_untouched(hip_lib):
    """Every refusal is decided before a device is touched (a renderer's device resources come with its first render), so all
    but the camera table's length -- a table needs a device; tests/test_gpu_render_pipeline.py -- are checked here."""
    lib, vp = hip_lib, _lib.vp
    K = np.array([100, 0, 32, 0, 100, 24, 0, 0, 1], np.float32)
    frames = np.full((2, 8, 8), 0xABCD, np.uint16)
    masks = np.full((2, 8, 8), 0xEE, np.uint8)
    meshes = (C.c_void_p * 1)(None)
    rd = C.c_void_p()
    assert lib.dh_renderer_create(0, C.byref(rd)) == 0 and rd.value

    def params(noise=0, holes=0.0):
        return _lib.RenderParams(noise, 0, holes, 7, (C.c_uint64 * 2)(0, 0))

    def inst(frame=0, mesh=0):
        a = np.zeros(1, _lib.RENDER_INSTANCE_DTYPE)
        a["frame"], a["mesh"] = frame, mesh
        return a

    def calls(r, ins, n, w, h, prm, fr=frames):
        p = C.byref(prm) if prm is not None else None
        ni = 0 if ins is None else len(ins)
        yield "dh_render_depth", lib.dh_render_depth(r, meshes, 1, vp(ins), ni, n, w, h, vp(K), p, vp(fr), vp(masks))
        yield "dh_render_depth_device", lib.dh_render_depth_device(r, meshes, 1, vp(ins), ni, n, w, h, vp(K), p, vp(fr), vp(masks), None)

    def refused(what, *args, **kw):
        for name, rc in calls(*args, **kw):
            assert rc == EINVAL and what in _err(lib) and name in _err(lib), (name, rc, _err(lib))
        assert (frames == 0xABCD).all() and (masks == 0xEE).all()

    refused("NULL renderer", None, None, 2, 8, 8, params())
    refused("NULL frames", rd, None, 2, 8, 8, params(), fr=None)
    refused("names frame 2 of 2", rd, inst(frame=2), 2, 8, 8, params())
    refused("names frame 4294967295 of 2", rd, inst(frame=0xFFFFFFFF), 2, 8, 8, params())
    refused("names mesh 1 of 1", rd, inst(mesh=1), 2, 8, 8, params())
    refused("mesh 0 is NULL", rd, inst(), 2, 8, 8, params())
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, _lib.RENDER_MAX_SIZE + 1), (_lib.RENDER_MAX_SIZE + 1, 8)):
        refused("frame size", rd, None, 2, w, h, params())
    for n in (0, -1, 65536):
        refused("frames", rd, None, n, 8, 8, params())
    for p in (-0.01, 1.0000001, np.nan, np.inf):
        refused("hole_probability", rd, None, 2, 8, 8, params(holes=p))
    refused("noise_amplitude", rd, None, 2, 8, 8, params(noise=65536))
    for name, fn in (("dh_render_depth_cameras", lib.dh_render_depth_cameras), ("dh_render_depth_cameras_device", lib.dh_render_depth_cameras_device)):
        extra = (None,) if name.endswith("_device") else ()
        assert fn(rd, meshes, 1, None, 0, 2, 8, 8, None, C.byref(params()), vp(frames), vp(masks), *extra) == EINVAL
        assert "NULL camera table" in _err(lib) and name in _err(lib)
        assert fn(None, meshes, 1, None, 0, 2, 8, 8, None, C.byref(params()), vp(frames), vp(masks), *extra) == EINVAL
    for name, rc in (("dh_render_depth", lib.dh_render_depth(rd, meshes, 1, None, 0, 2, 8, 8, None, None, vp(frames), vp(masks))),):
        assert rc == EINVAL and "NULL K" in _err(lib)
    assert (frames == 0xABCD).all() and (masks == 0xEE).all()
    assert lib.dh_renderer_timing(rd, (C.c_float * 4)()) == -6 and "profiling" in _err(lib)      # DH_ESTATE: nothing timed yet
    assert lib.dh_renderer_destroy(rd) == 0
