"""Every host form of a Fitter's nine methods driven without a GPU and without the library: the fitter is
made with object.__new__ and gets a recording stand-in for the library, whose every attribute is a function that notes (name,
arguments) and returns 0.  `host_cases` is the list of calls -- each kind with K and, where it has that form, with a camera table,
every nullable input once present and once None, no instances once, scores both ways -- and `describe` puts a recorded call into
words that do not depend on where an array lies: tools/fit_binding_trace.py prints them for two trees to be compared, and
tests/test_fit_binding.py holds them to the header."""
import ctypes as C
import hashlib

import numpy as np

W, H = 7, 5


class Recorder:
    """The library's stand-in: `calls` is [(name, args)] in call order."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def export(*args):
            self.calls.append((name, args))
            return 0
        return export


class Handle:
    """What a call reads of a Model, Views, Subjects, ShapeBasis or Cameras: its handle and its length."""

    def __init__(self, handle, n=0):
        self._h, self.n = C.c_void_p(handle), n

    def __len__(self):
        return self.n


class TracingNumpy:
    """numpy, with every array that ascontiguousarray, zeros and full return kept under its address: put in place of a module's
    `np`, it says which array lies behind a pointer the module passes on."""

    def __init__(self):
        self.made = {}

    def __getattr__(self, name):
        plain = getattr(np, name)
        if name not in ("ascontiguousarray", "zeros", "full"):
            return plain

        def traced(*args, **kw):
            out = plain(*args, **kw)
            self.made[out.ctypes.data] = out
            return out
        return traced


def fitter(fit, recorder):
    f = object.__new__(fit.Fitter)
    f._lib, f._h, f.device = recorder, C.c_void_p(1), 0
    return f


def host_cases(fit, _lib):
    """[(label, call)]: call(fitter) makes one host call.  Three cameras of W x H, two sets, five instances, three subjects."""
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 4000, (3, H, W)).astype(np.uint16)
    sets2 = rng.integers(0, 4000, (2, 3, H, W)).astype(np.uint16)
    K = np.array([[500.0, 0, W / 2], [0, 500.0, H / 2], [0, 0, 1]])
    cams, views, model, basis, subjects = Handle(2, 3), Handle(3, 3), Handle(4), Handle(5, 4), Handle(6, 3)
    models = [Handle(7), Handle(8)]

    def records(dtype, count):
        return np.frombuffer(rng.bytes(count * dtype.itemsize), dtype=dtype).copy()

    inst, vinst = records(_lib.RENDER_INSTANCE_DTYPE, 5), records(_lib.VIEW_INSTANCE_DTYPE, 5)
    frec, vfrec = records(_lib.FIT_RECORD_DTYPE, 5), records(_lib.VIEW_FIT_RECORD_DTYPE, 5)
    words = [int(v) for v in rng.integers(0, 3, 5)]                  # a list: the call makes the u32 array
    sets, take = np.array([0, 1, 1, 0, 1], np.int64), np.array([0, _lib.CALIB_SKIP, 0, 0, 0], np.uint32)
    enrolled, hold = [0, 5, 1], np.array([0, 1, 0], np.uint8)        # 5: the host form passes 1
    prm = {name: getattr(_lib, name)() for name in ("FitParams", "ShapeParams", "SurfaceParams", "IdentParams", "CalibParams")}
    for p in prm.values():
        C.memset(C.byref(p), 0x5A, C.sizeof(p))
    out = []
    for k, Karg in (("K", K), ("cameras", cams)):
        out += [(f"fit {k}", lambda f, Karg=Karg: f.fit(frames, models, inst, Karg)),
                (f"fit {k} params, no instances", lambda f, Karg=Karg: f.fit(frames, models[:1], inst[:0], Karg, params=prm["FitParams"])),
                (f"fit {k} no models", lambda f, Karg=Karg: f.fit(frames, [], inst[:1], Karg)),
                (f"shape {k}", lambda f, Karg=Karg: f.shape_step(frames, model, basis, inst, Karg)),
                (f"shape {k} subjects, params", lambda f, Karg=Karg: f.shape_step(frames, model, basis, inst, Karg, subjects=words, n_subjects=3,
                                                                                  params=prm["ShapeParams"])),
                (f"shape {k} no instances", lambda f, Karg=Karg: f.shape_step(frames, model, basis, inst[:0], Karg, n_subjects=0))]
        for name, method, p in (("shape_set", "shape_step_subjects", "ShapeParams"), ("surface", "surface_step_subjects", "SurfaceParams")):
            out += [(f"{name} {k}", lambda f, Karg=Karg, method=method: getattr(f, method)(frames, subjects, inst, Karg)),
                    (f"{name} {k} subjects", lambda f, Karg=Karg, method=method: getattr(f, method)(frames, subjects, inst, Karg, subjects=words, n_subjects=2)),
                    (f"{name} {k} fit_records, params", lambda f, Karg=Karg, method=method, p=p: getattr(f, method)(
                        frames, subjects, inst, Karg, fit_records=frec, params=prm[p])),
                    (f"{name} {k} no instances", lambda f, Karg=Karg, method=method: getattr(f, method)(frames, subjects, inst[:0], Karg, subjects=[],
                                                                                                        fit_records=frec[:0]))]
        out += [(f"ident {k}", lambda f, Karg=Karg: f.identify_subjects(frames, subjects, inst, Karg)),
                (f"ident {k} scores", lambda f, Karg=Karg: f.identify_subjects(frames, subjects, inst, Karg, n_subjects=2, scores=True)),
                (f"ident {k} enrolled", lambda f, Karg=Karg: f.identify_subjects(frames, subjects, inst, Karg, enrolled=enrolled, params=prm["IdentParams"])),
                (f"ident {k} fit_records, scores", lambda f, Karg=Karg: f.identify_subjects(frames, subjects, inst, Karg, fit_records=frec, scores=True)),
                (f"ident {k} no instances, scores", lambda f, Karg=Karg: f.identify_subjects(frames, subjects, inst[:0], Karg, scores=True))]
    out += [("fit_views", lambda f: f.fit_views(frames, models, vinst, views)),
            ("fit_views params, no instances", lambda f: f.fit_views(frames, models[:1], vinst[:0], views, params=prm["FitParams"])),
            ("shape_views", lambda f: f.shape_step_views(sets2, views, model, basis, vinst)),
            ("shape_views sets", lambda f: f.shape_step_views(sets2, views, model, basis, vinst, sets=sets, n_subjects=3)),
            ("shape_views subjects, params", lambda f: f.shape_step_views(sets2, views, model, basis, vinst, subjects=words, params=prm["ShapeParams"])),
            ("shape_views no instances", lambda f: f.shape_step_views(sets2, views, model, basis, vinst[:0], sets=[], subjects=[])),
            ("ident_views", lambda f: f.identify_subjects_views(sets2, views, subjects, vinst)),
            ("ident_views sets, scores", lambda f: f.identify_subjects_views(sets2, views, subjects, vinst, sets=sets, n_subjects=2, scores=True)),
            ("ident_views enrolled", lambda f: f.identify_subjects_views(sets2, views, subjects, vinst, enrolled=enrolled, params=prm["IdentParams"])),
            ("ident_views fit_records, scores", lambda f: f.identify_subjects_views(sets2, views, subjects, vinst, fit_records=vfrec, scores=True)),
            ("ident_views no instances", lambda f: f.identify_subjects_views(sets2, views, subjects, vinst[:0])),
            ("calib", lambda f: f.calibrate_step(sets2, views, model, vinst)),
            ("calib sets", lambda f: f.calibrate_step(sets2, views, model, vinst, sets=sets, params=prm["CalibParams"])),
            ("calib take", lambda f: f.calibrate_step(sets2, views, model, vinst, take=take)),
            ("calib hold", lambda f: f.calibrate_step(sets2, views, model, vinst, hold=hold)),
            ("calib no instances", lambda f: f.calibrate_step(sets2, views, model, vinst[:0]))]
    return out


def _array(a):
    return f"{a.dtype} {a.shape} {hashlib.sha1(a.tobytes()).hexdigest()}"


def describe(arg, made):
    """One argument of a recorded call in words: its ctypes kind, its scalar value and, for a pointer to numpy data (`made`: the
    arrays by address), the dtype, the shape and a digest of the bytes behind it."""
    if arg is None:
        return "NULL"
    if isinstance(arg, bool) or not isinstance(arg, (int, C.c_uint32, C.c_void_p, C.Array)) and type(arg).__name__ != "CArgObject":
        return f"UNEXPECTED {type(arg).__name__} {arg!r}"
    if isinstance(arg, int):
        return f"int {arg}"
    if isinstance(arg, C.c_uint32):
        return f"c_uint32 {arg.value}"
    if isinstance(arg, C.Array):
        return f"{type(arg).__name__} {list(arg)}"
    if isinstance(arg, C.c_void_p):
        behind = made.get(arg.value)
        return f"c_void_p -> {_array(behind)}" if behind is not None else f"c_void_p {arg.value}"
    return f"byref {type(arg._obj).__name__} {bytes(arg._obj).hex()}"


def result(out):
    """What a host call returned, in words."""
    return " | ".join(_array(o) for o in (out if isinstance(out, tuple) else (out,)))
