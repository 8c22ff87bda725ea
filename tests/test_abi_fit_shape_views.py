"""The multi-view shape entry points without a GPU: exported and declared, and every refusal that is decided
before a device is touched answers DH_EINVAL with a message that names the call and leaves the records untouched.  Models, bases
and view tables live on a device, so where a refusal only needs a handle that is not NULL the calls get a block that reads as
one: zeros for a model and a basis (0 points on device 0), and for the view table two words and a pointer (device, n cameras,
its camera table: again two words, device and n) -- every refusal tested here is decided before the handle's device memory would
be used.  The refusals that need a real model or basis (the extent, the field limit, the term limits) are in
tests/test_gpu_fit_shape_views.py."""
import ctypes as C
import re

import numpy as np

import abi_kit
from abi_kit import err as _err, Cameras as FakeCameras, Views as FakeViews
from depthhead_amd import _lib

NEW = ["dh_fit_shape_views", "dh_fit_shape_views_device"]
EINVAL = -1


def test_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    from depthhead_amd import fit
    assert callable(fit.Fitter.shape_step_views) and callable(fit.adapt_views)


def test_header_and_exports_are_equal():
    text = abi_kit.header()
    abi_kit.assert_header_equals_exports(NEW, "adapting a model's shape across views", "COUNTS PAIRS")
    # the two declarations differ in the stream alone
    host = re.search(r"int dh_fit_shape_views\((.*?)\);", text, re.S).group(1)
    device = re.search(r"int dh_fit_shape_views_device\((.*?)\);", text, re.S).group(1)
    assert " ".join(device.split()) == " ".join(host.split()) + ", void *stream"


def test_refusals_leave_the_records_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    frames = np.full((2, 3, 8, 8), 800, np.uint16)
    rec = np.full(2 * 88, 0xCD, np.uint8)
    zeros = np.zeros(256, np.uint8)
    cams = FakeCameras(0, 3)
    table = FakeViews(0, 3, C.addressof(cams))
    views = C.addressof(table)
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value

    def inst(first_cam=0, mask=0b111):
        a = np.zeros(1, _lib.VIEW_INSTANCE_DTYPE)
        a["first_cam"], a["views"], a["scale"] = first_cam, mask, 1.0
        a["R"][0] = np.eye(3, dtype=np.float32).reshape(9)
        a["t"][0] = (0, 0, 800)
        return a

    def calls(f, ins, n_sets, w, h, prm, fr=frames, r=rec, vw=views, mdl=zeros, bas=zeros, sets=None, subj=None, ns=1, device_too=True, ni=None):
        p = C.byref(prm) if prm is not None else None
        ni = (0 if ins is None else len(ins)) if ni is None else ni
        yield "dh_fit_shape_views", lib.dh_fit_shape_views(f, vp(fr), n_sets, w, h, vp(vw), vp(mdl), vp(bas), vp(ins), ni, vp(sets), vp(subj), ns, p, vp(r))
        if device_too:
            yield "dh_fit_shape_views_device", lib.dh_fit_shape_views_device(f, vp(fr), n_sets, w, h, vp(vw), vp(mdl), vp(bas), vp(ins), ni, vp(sets),
                                                                             vp(subj), ns, p, vp(r), None)

    def refused(what, *args, **kw):
        for name, rc in calls(*args, **kw):
            assert rc == EINVAL and what in _err(lib) and name + ":" in _err(lib), (name, rc, _err(lib))
        assert (rec == 0xCD).all()

    def default_params():
        p = _lib.ShapeParams()
        assert lib.dh_shape_params_default(C.byref(p)) == 0
        return p

    prm = default_params()
    refused("NULL fitter", None, None, 2, 8, 8, prm)
    refused("NULL frames", ft, None, 2, 8, 8, prm, fr=None)
    refused("NULL records", ft, None, 2, 8, 8, prm, r=None)
    refused("NULL model", ft, None, 2, 8, 8, prm, mdl=None)
    refused("NULL basis", ft, None, 2, 8, 8, prm, bas=None)
    refused("NULL view table", ft, None, 2, 8, 8, prm, vw=None)
    elsewhere = FakeViews(1, 3, C.addressof(cams))
    refused("the view table lives on device 1", ft, None, 2, 8, 8, prm, vw=C.addressof(elsewhere))
    refused("n_sets = 0", ft, None, 0, 8, 8, prm)
    refused("n_sets = 21846", ft, None, 21846, 8, 8, prm)                 # 21846 * 3 = 65538; 21845 * 3 = 65535 passes this test
    refused("frame size", ft, None, 21845, 0, 8, prm)
    refused("n_sets = 4294967295", ft, None, 0xFFFFFFFF, 8, 8, prm)
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, _lib.RENDER_MAX_SIZE + 1), (_lib.RENDER_MAX_SIZE + 1, 8)):
        refused("frame size", ft, None, 2, w, h, prm)
    for ns in (0, 257, 0xFFFFFFFF):
        refused("n_subjects", ft, None, 2, 8, 8, prm, ns=ns)

    def with_params(**kw):
        p = default_params()
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    for v in (0.0, -1.0, 256.5, np.nan, np.inf):
        refused("gate", ft, None, 2, 8, 8, with_params(gate=v))
    for v in (-1e-9, np.nan, np.inf):
        refused("lambda", ft, None, 2, 8, 8, with_params(lam=v))
    refused("min_points 0", ft, None, 2, 8, 8, with_params(min_points=0))
    for kw in (dict(reserved0=1), dict(reserved=0), dict(reserved=1)):
        refused("reserved", ft, None, 2, 8, 8, with_params(**kw))
    refused("NULL instances", ft, None, 2, 8, 8, None, ni=1)
    refused("too many instances", ft, inst(), 2, 8, 8, None, ni=(1 << 23) + 1)
    # the host form's per-instance refusals (the _device form cannot read the instances: the device skips these)
    host = dict(device_too=False)
    refused("instance 0 is seen by no view", ft, inst(mask=0), 2, 8, 8, prm, **host)
    refused("names camera 3 of 3", ft, inst(mask=0b1000), 2, 8, 8, prm, **host)
    refused("names camera 3 of 3", ft, inst(first_cam=2, mask=0b11), 2, 8, 8, prm, **host)
    refused("names camera 63 of 3", ft, inst(mask=(1 << 63) | 1), 2, 8, 8, prm, **host)
    refused("names camera 4294967296 of 3", ft, inst(first_cam=0xFFFFFFFF, mask=0b10), 2, 8, 8, prm, **host)
    refused("names set 2 of 2", ft, inst(), 2, 8, 8, prm, sets=np.array([2], np.uint32), **host)
    refused("names set 4294967295 of 2", ft, inst(), 2, 8, 8, prm, sets=np.array([0xFFFFFFFF], np.uint32), **host)
    refused("names subject 1 of 1", ft, inst(), 2, 8, 8, prm, subj=np.array([1], np.uint32), **host)
    refused("names subject 4294967294 of 1", ft, inst(), 2, 8, 8, prm, subj=np.array([0xFFFFFFFE], np.uint32), **host)
    # the order: the view, the camera, the set, the subject, then R, t and scale
    bad = inst(mask=0)
    bad["R"][0, 0] = np.nan
    refused("seen by no view", ft, bad, 2, 8, 8, prm, sets=np.array([9], np.uint32), subj=np.array([9], np.uint32), **host)
    bad["views"] = 0b1000
    refused("names camera 3", ft, bad, 2, 8, 8, prm, sets=np.array([9], np.uint32), subj=np.array([9], np.uint32), **host)
    bad["views"] = 0b1
    refused("names set 9", ft, bad, 2, 8, 8, prm, sets=np.array([9], np.uint32), subj=np.array([9], np.uint32), **host)
    refused("names subject 9", ft, bad, 2, 8, 8, prm, subj=np.array([9], np.uint32), **host)
    refused("non-finite R, t or scale", ft, bad, 2, 8, 8, prm, **host)
    for field, idx in (("R", 4), ("t", 2), ("scale", None)):
        for x in (np.nan, np.inf, -np.inf):
            a = inst()
            if idx is None:
                a[field][0] = x
            else:
                a[field][0, idx] = x
            refused("non-finite R, t or scale", ft, a, 2, 8, 8, prm, **host)
    for idx, x, where in ((7, -2.5, "[1][2]"), (0, 1.011, "[0][0]"), (1, 0.021, "[0][1]")):
        a = inst()
        a["R"][0, idx] = x
        refused(f"not orthonormal: (R R^T){where}", ft, a, 2, 8, 8, prm, **host)
    assert (rec == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0
