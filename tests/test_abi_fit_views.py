"""The multi-view fit's entry points without a GPU: exported and declared, header and _lib.EXPORTS equal,
the dh_view_instance / dh_view_fit_record layouts of the Python side equal the C layout (a g++ program prints sizeof and offsetof
from include/depthhead_hip.h), the refusals that need no device, and fit.views_from_rig.  A view table is bound to a camera
table, which lives on a device: every refusal that comes after "NULL view table" in the header's order -- the frame size, the
params, the per-instance ones, dh_fit_views_create's own -- is in tests/test_gpu_fit_views.py."""
import ctypes as C

import numpy as np
import pytest

import abi_kit
from abi_kit import err as _err
from depthhead_amd import _lib, fit

NEW = ["dh_fit_views_create", "dh_fit_views_destroy", "dh_fit_views_info", "dh_fit_depth_views", "dh_fit_depth_views_device"]
EINVAL = -1

LAYOUT_CPP = r"""
#include <stddef.h>
#include <stdio.h>
#include "depthhead_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main() {
    printf("dh_view_instance size %zu\n", sizeof(dh_view_instance));
    F(dh_view_instance, first_cam); F(dh_view_instance, model); F(dh_view_instance, views); F(dh_view_instance, R);
    F(dh_view_instance, t); F(dh_view_instance, scale); F(dh_view_instance, flags);
    printf("dh_view_fit_record size %zu\n", sizeof(dh_view_fit_record));
    F(dh_view_fit_record, points); F(dh_view_fit_record, steps); F(dh_view_fit_record, status); F(dh_view_fit_record, reserved);
    F(dh_view_fit_record, sum_r2_fixed); F(dh_view_fit_record, views_used);
    printf("consts %.17g %d\n", (double)DH_FIT_VIEW_TOLERANCE, (int)DH_FIT_MAX_POINTS);
    return 0;
}
"""


def test_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    for name in ("Views", "views_from_rig", "view_instances_from_persons"):
        assert callable(getattr(fit, name)), name
    assert callable(fit.Fitter.fit_views)
    assert fit.VIEW_INSTANCE_DTYPE is _lib.VIEW_INSTANCE_DTYPE and fit.VIEW_FIT_RECORD_DTYPE is _lib.VIEW_FIT_RECORD_DTYPE


def test_header_and_exports_are_equal():
    abi_kit.assert_header_equals_exports(NEW)


def test_layouts_match_the_header(tmp_path):
    c, consts = abi_kit.layouts(tmp_path, LAYOUT_CPP)
    assert float(consts[0]) == _lib.FIT_VIEW_TOLERANCE == 0.001 and int(consts[1]) == _lib.FIT_MAX_POINTS
    for name, dt, size in (("dh_view_instance", _lib.VIEW_INSTANCE_DTYPE, 72), ("dh_view_fit_record", _lib.VIEW_FIT_RECORD_DTYPE, 32)):
        assert c[(name, "size")] == dt.itemsize == size
        for f in dt.names:
            assert c[(name, f)] == dt.fields[f][1], (name, f)
        assert sum(dt.fields[f][0].itemsize for f in dt.names) == size, name          # no padding


def test_refusals_that_need_no_device(hip_lib):
    lib, vp = hip_lib, _lib.vp
    frames = np.full((2, 8, 8), 800, np.uint16)
    out = np.full(72, 0xAB, np.uint8)
    rec = np.full(32, 0xCD, np.uint8)
    inst = np.zeros(1, _lib.VIEW_INSTANCE_DTYPE)
    models = (C.c_void_p * 1)(None)
    h = C.c_void_p(1234)
    V, u = np.eye(3, dtype=np.float32).reshape(1, 9), np.zeros((1, 3), np.float32)
    assert lib.dh_fit_views_create(None, vp(V), vp(u), C.byref(h)) == EINVAL and "NULL" in _err(lib) and h.value is None
    assert lib.dh_fit_views_create(None, vp(V), vp(u), None) == EINVAL and "NULL" in _err(lib)
    assert lib.dh_fit_views_destroy(None) == 0
    assert lib.dh_fit_views_info(None, None, None) == EINVAL and "NULL view table" in _err(lib)
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value
    fake = C.c_void_p(8)                    # never read: each refusal below is decided before the view table is looked at

    def calls(f, fr, o, r, views):
        yield "dh_fit_depth_views", lib.dh_fit_depth_views(f, vp(fr), 8, 8, views, models, 1, vp(inst), 1, None, vp(o), vp(r))
        yield "dh_fit_depth_views_device", lib.dh_fit_depth_views_device(f, vp(fr), 8, 8, views, models, 1, vp(inst), 1, None, vp(o), vp(r), None)

    for what, args in (("NULL fitter", (None, frames, out, rec, fake)), ("NULL frames", (ft, None, out, rec, fake)),
                       ("NULL output", (ft, frames, None, rec, fake)), ("NULL output", (ft, frames, out, None, fake)),
                       ("NULL view table", (ft, frames, out, rec, None))):
        for name, rc in calls(*args):
            assert rc == EINVAL and what in _err(lib) and name in _err(lib), (name, rc, _err(lib))
    assert (out == 0xAB).all() and (rec == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0


def test_views_from_rig_round_trip_and_refusal():
    from depthhead_amd import render
    rs = np.random.RandomState(3)
    R = np.stack([render.euler_to_matrix(a).astype(np.float64) for a in ((10, -35, 4), (0, 0, 0), (-7, 35, 12), (170, 80, -100))])
    t = rs.uniform(-1500, 1500, (4, 3))
    V, u = fit.views_from_rig(R, t)
    assert V.dtype == u.dtype == np.float32 and V.shape == (4, 3, 3) and u.shape == (4, 3)
    assert V.tobytes() == np.transpose(R, (0, 2, 1)).astype(np.float32).tobytes()
    assert u[1].tolist() == (-t[1]).astype(np.float32).tolist()
    m = rs.uniform(-300, 300, (50, 3))                                   # camera-space points
    for c in range(4):
        world = m @ R[c].T + t[c]                                        # R m + t
        back = world @ V[c].astype(np.float64).T + u[c]                  # V (R m + t) + u
        # f32 rounding of V and u at |world| and |u| up to 3000 mm: 3 * 2^-24 * 3000 * sqrt(3) + 2^-24 * 3000 < 1.3e-3 mm
        assert np.abs(back - m).max() < 1.3e-3, c
    assert fit.views_from_rig(R.reshape(4, 9), t)[0].tobytes() == V.tobytes()
    bad = R.copy()
    bad[2, 0, 0] += 0.002                                                # (R R^T)[0][0] off by more than 1e-3
    with pytest.raises(ValueError, match="camera 2"):
        fit.views_from_rig(bad, t)
    with pytest.raises(ValueError, match="camera 0"):
        fit.views_from_rig(R * np.array([1.0, 1.0, -1.0]), t)            # a reflection
    with pytest.raises(ValueError):
        fit.views_from_rig(R, t[:3])
    nan = R.copy()
    nan[1, 1, 1] = np.nan
    with pytest.raises(ValueError, match="camera 1"):
        fit.views_from_rig(nan, t)


def test_view_instances_from_persons_on_hand_made_records():
    """Shape and sanity only: the helper is outside the bit-exact contract."""
    from depthhead_amd import render, tracking
    persons = np.zeros(2, _lib.RIG_PERSON_DTYPE)
    heads = np.zeros((5, 4), _lib.HEAD_DTYPE)
    persons["world"] = [(10.0, -20.0, 30.0), (-300.0, 5.0, 120.0)]
    persons["views"], persons["best_cam"], persons["best_head"] = [0b011, 0b100], [3, 4], [1, 0]
    heads[3, 1]["pose"]["rotation"] = (0.1, -0.3, 0.05)
    heads[4, 0]["pose"]["rotation"] = (-0.2, 0.4, 0.0)
    rig_R = np.stack([render.euler_to_matrix((0, 20.0 * c, 0)).astype(np.float64) for c in range(5)])
    inst = fit.view_instances_from_persons(persons, heads, rig_R, np.zeros((5, 3)), 2, scale=0.9, model=3)
    assert inst.dtype == _lib.VIEW_INSTANCE_DTYPE and len(inst) == 2
    assert inst["first_cam"].tolist() == [2, 2] and inst["views"].tolist() == [0b011, 0b100] and inst["model"].tolist() == [3, 3]
    assert inst["t"].tolist() == persons["world"].tolist() and np.allclose(inst["scale"], 0.9) and not inst["flags"].any()
    for i, (cam, hd) in enumerate(((3, 1), (4, 0))):
        want = tracking.world_rotation(rig_R[cam], heads[cam, hd]["pose"]["rotation"])
        assert inst["R"][i].tobytes() == want.astype(np.float32).reshape(9).tobytes()
        assert np.abs(want @ want.T - np.eye(3)).max() < 1e-6
