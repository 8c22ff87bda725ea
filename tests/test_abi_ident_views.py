"""The multi-view identification entry points without a GPU: exported and declared, the argument lists of the
two forms, the two defaults, and every refusal that is decided before a device is touched, in the header's order with every later
one provoked as well, answering DH_EINVAL with a message that names the call and leaving the four outputs untouched.  Handles live
on a device, so the calls get blocks that read as one (dh_api_fit.hip): a view table of two words and a pointer to its camera table
(device, n), and a subject set (device; n, n_tris, n_subjects; max_coeff, radius; its basis: device; n, k; largest) whose device
memory is never touched -- every refusal made here comes before the set's models are read.  What needs a real set and a real rig
is in tests/test_gpu_ident_views.py."""
import ctypes as C
import re

import numpy as np

import abi_kit
from abi_kit import err as _err, Basis as FakeBasis, Cameras as FakeCameras, SubjectSet as FakeSet, Views as FakeViews
from depthhead_amd import _lib

NEW = ["dh_fit_ident_views_params_default", "dh_fit_identify_subjects_views", "dh_fit_identify_subjects_views_device"]
EINVAL = -1


def test_entry_points_are_exported(hip_lib):
    abi_kit.assert_exported(hip_lib, NEW)
    from depthhead_amd import fit
    for name in ("recognise_subjects_views", "ident_views_params"):
        assert callable(getattr(fit, name)), name
    assert callable(fit.Fitter.identify_subjects_views)


def test_header_and_exports_are_equal():
    abi_kit.assert_header_equals_exports(NEW, "identifying enrolled subjects across the views of a rig", "MUST BE STREAM-ORDERED")


def test_the_argument_lists():
    """The two declarations differ in the stream alone; the order is dh_fit_shape_views' up to `sets` (the set in place of the model
    and its basis), then section 27's from `enrolled` on, with the view types for the instances, the fit records, poses and scores."""
    args = abi_kit.declared_args
    host, device = args("dh_fit_identify_subjects_views"), args("dh_fit_identify_subjects_views_device")
    assert device == host + ["void *stream"]
    shape, ident = args("dh_fit_shape_views"), args("dh_fit_identify_subjects_cameras")
    upto = shape.index("const uint32_t *sets") + 1
    assert "dh_fit_model" in shape[6] and "dh_fit_basis" in shape[7]
    head = shape[:6] + ["const dh_fit_subjects *set"] + shape[8:upto]
    assert host[:len(head)] == head
    swap = {"dh_render_instance": "dh_view_instance", "dh_fit_record": "dh_view_fit_record"}
    tail = ident[ident.index("const uint8_t *enrolled"):]
    for old, new in swap.items():
        tail = [a.replace(old, new) for a in tail]
    assert host[len(head):] == tail
    assert C.sizeof(C.c_uint64) * 4 == _lib.VIEW_FIT_RECORD_DTYPE.itemsize == 32 and _lib.VIEW_INSTANCE_DTYPE.itemsize == 72


def test_the_two_defaults(hip_lib):
    p, q = _lib.IdentParams(), _lib.IdentParams()
    C.memset(C.byref(p), 0xCD, C.sizeof(p))
    C.memset(C.byref(q), 0xCD, C.sizeof(q))
    assert hip_lib.dh_fit_ident_views_params_default(C.byref(p)) == 0 and hip_lib.dh_fit_ident_params_default(C.byref(q)) == 0
    assert (p.iterations, p.min_points, p.gate, p.lam, p.max_rms, p.min_ratio, p.reserved[0], p.reserved[1], p.reserved[2]) == \
        (4, 64, 25.0, 1e-3, _lib.IDENT_VIEWS_DEFAULT_MAX_RMS, 1.0, 0, 0, 0)
    assert q.max_rms == _lib.IDENT_DEFAULT_MAX_RMS == 1.68                          # section 27's stays what it was
    q.max_rms = p.max_rms
    assert bytes(p) == bytes(q)                                                     # max_rms is the one difference
    text = abi_kit.header()
    assert float(re.search(r"#define DH_IDENT_VIEWS_DEFAULT_MAX_RMS\s+([0-9.]+)", text).group(1)) == _lib.IDENT_VIEWS_DEFAULT_MAX_RMS
    assert hip_lib.dh_fit_ident_views_params_default(None) == EINVAL and "NULL" in _err(hip_lib)
    from depthhead_amd import fit
    r = fit.ident_views_params(iterations=7, min_points=9, gate=30.0, lam=0.5, min_ratio=1.25)
    assert (r.iterations, r.min_points, r.gate, r.lam, r.max_rms, r.min_ratio) == (7, 9, 30.0, 0.5, _lib.IDENT_VIEWS_DEFAULT_MAX_RMS, 1.25)
    assert fit.ident_views_params(max_rms=np.inf).max_rms == np.inf


def bad_params(reserved=0, **kw):
    p = _lib.IdentParams()
    assert _lib.load().dh_fit_ident_views_params_default(C.byref(p)) == 0
    for name, value in kw.items():
        setattr(p, name, value)
    p.reserved[0] = reserved
    return p


def test_refusals_in_their_order_leave_the_outputs_untouched(hip_lib):
    lib, vp = hip_lib, _lib.vp
    frames = np.full((2, 3, 8, 8), 800, np.uint16)
    out = {name: np.full(512, 0xCD, np.uint8) for name in ("sub", "rec", "poses", "scores")}
    ft = C.c_void_p()
    assert lib.dh_fitter_create(0, C.byref(ft)) == 0 and ft.value
    cams, cams1 = FakeCameras(0, 3), FakeCameras(1, 3)
    table, elsewhere = FakeViews(0, 3, C.addressof(cams)), FakeViews(1, 3, C.addressof(cams1))
    basis = FakeBasis(0, 642, 1, 0, 10.0)
    keep = [cams, cams1, table, elsewhere, basis]

    def a_set(device=0, n=642, n_subjects=3, radius=100.0):
        s = FakeSet(device, n, 1280, n_subjects, 0.5, radius, C.addressof(basis))
        keep.append(s)
        return C.addressof(s)

    def inst(first_cam=0, mask=0b111, count=1):
        a = np.zeros(count, _lib.VIEW_INSTANCE_DTYPE)
        a["first_cam"], a["views"], a["scale"] = first_cam, mask, 1.0
        a["R"][:] = np.eye(3, dtype=np.float32).reshape(9)
        a["t"][:] = (0, 0, 800)
        return a

    good = a_set()

    def calls(f=ft, fr=frames, vw=C.addressof(table), st=good, sub=out["sub"], rec=out["rec"], n_sets=2, w=8, h=8, ns=3, prm=None, instances=None,
              ni=None, sets=None, frec=None, device_too=True):
        """Both forms with the same arguments: (name, return code, message)."""
        ni = (0 if instances is None else len(instances)) if ni is None else ni
        args = (f, vp(fr), C.c_uint32(n_sets), w, h, vp(vw), vp(st), vp(instances), C.c_uint32(ni), vp(sets), None, C.c_uint32(ns), vp(frec),
                C.byref(prm) if prm is not None else None, vp(sub), vp(rec), vp(out["poses"]), vp(out["scores"]))
        for name, extra in (("dh_fit_identify_subjects_views", ()), ("dh_fit_identify_subjects_views_device", (None,)))[:2 if device_too else 1]:
            rc = getattr(lib, name)(*args, *extra)
            yield name, rc, _err(lib)

    def refused(text, **kw):
        for name, rc, msg in calls(**kw):
            assert rc == EINVAL and text in msg and name + ":" in msg, (name, rc, msg, text)
        for buf in out.values():
            assert (buf == 0xCD).all()

    # 1. the NULL pointers, each with every later refusal provoked as well
    later = dict(vw=C.addressof(elsewhere), n_sets=0, w=0, ns=0, prm=bad_params(gate=np.nan), ni=1, st=a_set(device=1))
    refused("NULL fitter", f=None, **later)
    refused("NULL frames", fr=None, **later)
    refused("NULL subjects_out", sub=None, **later)
    refused("NULL records", rec=None, **later)
    refused("NULL subject set", **dict(later, st=None))
    # 2. the view table, 3. n_sets and n_sets * n, 4. the frame size
    refused("NULL view table", **dict(later, vw=None))
    refused("the view table lives on device 1, the fitter on 0", **later)
    del later["vw"]
    refused("n_sets = 0", **later)
    for n_sets in (21846, 0xFFFFFFFF):                                              # 21846 * 3 = 65538; 21845 * 3 = 65535 passes this test
        refused(f"n_sets = {n_sets}", **dict(later, n_sets=n_sets))
    del later["n_sets"]
    refused("frame size", **dict(later, n_sets=21845))
    del later["w"]
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, _lib.RENDER_MAX_SIZE + 1), (_lib.RENDER_MAX_SIZE + 1, 8)):
        refused("frame size", w=w, h=h, **later)
    # 5. a set on another device, 6. n_subjects outside 1 .. S
    refused("the subject set lives on device 1, the fitter on 0", **later)
    del later["st"], later["ns"]
    for ns in (0, 4, 0xFFFFFFFF):
        refused(f"n_subjects = {ns}, expected 1 .. 3", ns=ns, **later)
    # 7. the parameters, in section 27's order, each with the later ones provoked as well
    del later["prm"]
    for kw in (dict(gate=np.nan), dict(lam=np.nan), dict(max_rms=np.nan), dict(min_ratio=np.nan)):
        refused("a value is NaN", prm=bad_params(**dict(dict(iterations=65, min_points=0), **kw)), **later)
    refused("iterations = 65 above 64", prm=bad_params(iterations=65, gate=0.0, lam=-1.0, min_points=5, max_rms=0.0, min_ratio=0.5, reserved=1), **later)
    for gate in (0.0, -1.0, 4096.5, np.inf):
        refused("gate", prm=bad_params(gate=gate, lam=-1.0, min_points=5, max_rms=0.0, min_ratio=0.5, reserved=1), **later)
    for lam in (-1e-9, np.inf):
        refused("lambda", prm=bad_params(lam=lam, min_points=5, max_rms=0.0, min_ratio=0.5, reserved=1), **later)
    refused("min_points 5 below 6", prm=bad_params(min_points=5, max_rms=0.0, min_ratio=0.5, reserved=1), **later)
    for rms in (0.0, -1.0, -np.inf):
        refused("max_rms", prm=bad_params(max_rms=rms, min_ratio=0.5, reserved=1), **later)
    for ratio in (0.999, 0.0, -np.inf):
        refused("min_ratio", prm=bad_params(min_ratio=ratio, reserved=1), **later)
    for word in range(3):
        p = bad_params()
        p.reserved[word] = 1
        refused("reserved", prm=p, **later)
    # 8. NULL instances, then 9. the pair limit (before any instance is read: this one is no instance that may take part)
    refused("NULL instances", ni=(1 << 22) + 1)
    refused(f"{(1 << 22) // 3 + 1} instances times 3 subjects exceed {1 << 22} pairs", instances=inst(mask=0), ni=(1 << 22) // 3 + 1)
    # 10. the host form, per instance: the six tests of taking part in their order, each with every later one provoked as well --
    # a set past n_sets, a fit record that is not DH_FIT_OK, a NaN in R, a scale past the extent and the field limit, and a set of
    # 16385 points, of which two views sum 32770 terms
    host = dict(device_too=False, st=a_set(n=16385), sets=np.array([9], np.uint32))
    frec = np.zeros(1, _lib.VIEW_FIT_RECORD_DTYPE)
    frec["status"] = 1
    bad = inst(mask=0)
    bad["R"][0, 0], bad["scale"] = np.nan, 1e6
    refused("instance 0 is seen by no view", instances=bad, frec=frec, **host)
    for first_cam, mask, named in ((0, 0b1000, 3), (2, 0b11, 3), (0, (1 << 63) | 1, 63), (0xFFFFFFFF, 0b10, 4294967296)):
        bad["first_cam"], bad["views"] = first_cam, mask
        refused(f"instance 0 names camera {named} of 3", instances=bad, frec=frec, **host)
    bad["first_cam"], bad["views"] = 0, 0b11
    refused("instance 0 names set 9 of 2", instances=bad, frec=frec, **host)
    refused("names set 4294967295 of 2", instances=bad, frec=frec, **dict(host, sets=np.array([0xFFFFFFFF], np.uint32)))
    host["sets"] = np.array([1], np.uint32)
    refused("non-finite R, t or scale", instances=bad, **host)                      # (with the fit record it would be skipped: no error)
    for field, idx in (("R", 4), ("t", 2), ("scale", None)):
        for x in (np.nan, np.inf, -np.inf):
            a = inst(mask=0b11)
            if idx is None:
                a[field][0] = x
            else:
                a[field][0, idx] = x
            refused("non-finite R, t or scale", instances=a, **host)
    a = inst(mask=0b11)
    a["R"][0, 7], a["scale"] = -2.5, 1e6
    refused("not orthonormal: (R R^T)[1][2]", instances=a, **host)
    a = inst(mask=0b11)
    a["scale"] = 41.0                                                               # 41 * 100 mm > 4096, and 41 * 10 > 256 as well
    refused("instance 0", instances=a, **host)
    assert "spans" in _err(lib), _err(lib)
    a["scale"] = 26.0                                                               # 2600 mm: inside the extent; 260 > 256: the field limit
    refused("instance 0", instances=a, **host)
    assert "spans" not in _err(lib), _err(lib)
    two = inst(mask=0b11, count=2)
    two["views"][1] = 0b101
    refused("instance 0 sums 32770 terms (2 views of 16385 points), above 32768", instances=two, sets=None, device_too=False, st=host["st"])
    two["views"][0] = 0b1                                                           # the first takes part, the second is refused
    refused("instance 1 sums 32770 terms", instances=two, sets=None, device_too=False, st=host["st"])
    # what is allowed: max_rms = +inf, iterations 0 and 64, no instances at all -- no error, nothing written
    for prm in (bad_params(max_rms=np.inf), bad_params(iterations=0), bad_params(iterations=64, min_points=6, gate=4096.0, lam=0.0), None):
        for name, rc, msg in calls(prm=prm, ni=0, instances=None):
            assert rc == 0, (name, msg)
    for buf in out.values():
        assert (buf == 0xCD).all()
    assert lib.dh_fitter_destroy(ft) == 0
