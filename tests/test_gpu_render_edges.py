"""The renderer on the GPU on the edge families of tests/render_families.py: (a) every case through the
host entry point, depth and mask equal to the restatement on every pixel of every frame, no tolerance; (b) the device twins
writing into the caller's memory -- outputs inside larger allocations between guard bands of seeded bytes, aligned and skewed
so that the pointer alone selects the narrow store path, with and without masks, on the default and on another stream, through
a test-local ctypes call shaped like render.Renderer.render's; (c) renderer state: a first call in which every triangle is
dropped, the deepest lists right after it, the same call twice and with its instances reversed."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import render_families as rf
import render_ref as rr
from depthhead_amd import _lib, render

pytestmark = pytest.mark.gpu

BAND = 4096                 # bytes of guard either side of an output


def to_gpu(items):
    return render.instances([(i["frame"], i["mesh"], i["R"], i["t"], float(i["scale"]), bool(i["flags"])) for i in items])


@contextlib.contextmanager
def gpu_meshes(c):
    ms = [render.Mesh(v, t) for v, t in c["meshes"]]
    try:
        yield ms
    finally:
        for m in ms:
            m.close()


@pytest.fixture(scope="module")
def renderer():
    with render.Renderer() as rd:
        yield rd


def compare(frames, masks, c):
    """Every pixel against the restatement; the first differing pixels and both values on failure."""
    want_f, want_m = rf.expected(c)
    assert frames.shape == want_f.shape and frames.dtype == np.uint16
    bad = np.argwhere(frames != want_f)
    assert bad.size == 0, (c["label"], len(bad), bad[:5].tolist(), [int(frames[tuple(b)]) for b in bad[:5]], [int(want_f[tuple(b)]) for b in bad[:5]])
    if masks is not None:
        bad = np.argwhere(masks != want_m)
        assert bad.size == 0, (c["label"], len(bad), bad[:5].tolist(), [int(masks[tuple(b)]) for b in bad[:5]], [int(want_m[tuple(b)]) for b in bad[:5]])


def draw(rd, ms, c, items=None):
    return rd.render(ms, to_gpu(c["instances"] if items is None else items), c["n"], c["w"], c["h"], c["K"], **c["sensor"])


# ------------------------------------------------------------------ (a) every family, host entry point
@pytest.mark.parametrize("label", rf.LABELS)
def test_family_on_the_host_entry_point(renderer, label):
    c = rf.all_cases()[label]
    c["reach"](rf.census(c))
    if c["K"].size == 9:
        with gpu_meshes(c) as ms:
            compare(*draw(renderer, ms, c), c)
    else:
        from depthhead_amd.tracking import Cameras
        with gpu_meshes(c) as ms, Cameras(c["K"].reshape(c["n"], 9)) as cams:
            compare(*renderer.render(ms, to_gpu(c["instances"]), c["n"], c["w"], c["h"], cams, **c["sensor"]), c)


# ------------------------------------------------------------------ (b) the device twins into the caller's memory
def pattern(nbytes, seed):
    """Seeded bytes, none of them zero."""
    return (rr.splitmix_at(seed, np.arange(nbytes, dtype=np.uint64)) % np.uint64(255) + np.uint64(1)).astype(np.uint8)


class Guarded:
    """`nbytes` of output inside a larger torch allocation: BAND bytes of pattern, the output `skew` bytes past a boundary of
    `align`, BAND bytes of pattern; the output itself holds the pattern too."""

    def __init__(self, nbytes, align, skew, seed):
        import torch
        self.host = pattern(nbytes + 2 * BAND + 2 * align, seed)
        self.buf = torch.from_numpy(self.host).cuda()
        self.off = BAND + (-(self.buf.data_ptr() + BAND)) % align + skew
        self.nbytes = nbytes
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % align == skew and self.off >= BAND and self.off + nbytes + BAND <= len(self.host)

    def read(self):
        """The output bytes, after checking that nothing around them changed."""
        back = self.buf.cpu().numpy()
        lo, hi = self.off, self.off + self.nbytes
        assert np.array_equal(back[:lo], self.host[:lo]), ("written before the output", np.argwhere(back[:lo] != self.host[:lo])[:5].ravel().tolist(), lo)
        assert np.array_equal(back[hi:], self.host[hi:]), ("written past the output", (np.argwhere(back[hi:] != self.host[hi:])[:5].ravel() + hi).tolist(), hi)
        return back[lo:hi].tobytes()


def render_into(rd, ms, c, frames_ptr, masks_ptr, stream, cams):
    """dh_render_depth_device / dh_render_depth_cameras_device as render.Renderer.render calls them, into the caller's pointers."""
    lib = _lib.load()
    inst = np.ascontiguousarray(to_gpu(c["instances"]), dtype=_lib.RENDER_INSTANCE_DTYPE)
    handles = (C.c_void_p * len(ms))(*[m._h.value for m in ms])
    s = c["sensor"]
    prm = _lib.RenderParams(int(s.get("noise", 0)), 0, float(s.get("holes", 0.0)), int(s.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF, (C.c_uint64 * 2)(0, 0))
    head = (rd._h, handles, C.c_uint32(len(ms)), _lib.vp(inst), C.c_uint32(len(inst)), c["n"], c["w"], c["h"])
    tail = (C.byref(prm), C.c_void_p(frames_ptr), C.c_void_p(masks_ptr) if masks_ptr else None, C.c_void_p(stream))
    if cams is None:
        K = np.ascontiguousarray(c["K"], dtype=np.float32).reshape(9)
        _lib.check(lib.dh_render_depth_device(*head, _lib.vp(K), *tail))
    else:
        _lib.check(lib.dh_render_depth_cameras_device(*head, cams._h, *tail))


def twin_case(w, sensor):
    h = {72: 16, 65: 17}[w]
    scene = "frame_shapes-%dx%dx2" % (w, h)
    if not sensor:
        return rf.all_cases()[scene]
    return rf.shape_case(scene + "-twin-sensor", w, h, 2, sensor={"noise": 2, "holes": 0.05, "seed": 77}, scene=scene)


# (w, bytes past a 16-byte boundary for the frames, bytes past an 8-byte boundary for the masks or None for masks = NULL,
#  camera table, another stream, sensor model).  72 % 8 == 0: there the skew alone must select the narrow path.
TWINS = [(72, 0, 0, False, False, False), (72, 2, 0, False, False, False), (72, 0, 1, True, False, False), (72, 2, 1, False, True, True),
         (72, 0, None, False, False, False), (72, 2, None, True, True, False), (72, 0, 0, True, True, True),
         (65, 0, 0, False, False, False), (65, 2, 1, True, False, True), (65, 0, 1, False, True, False), (65, 2, None, False, False, False)]


@pytest.mark.parametrize("w,fskew,mskew,table,side,sensor", TWINS)
def test_device_twins_write_the_output_and_nothing_else(renderer, w, fskew, mskew, table, side, sensor):
    import torch
    from depthhead_amd.tracking import Cameras
    c = twin_case(w, sensor)
    n_px = c["n"] * c["w"] * c["h"]
    want_f, want_m = rf.expected(c)
    frames = Guarded(2 * n_px, 16, fskew, 1000 + w)
    masks = Guarded(n_px, 8, mskew, 2000 + w) if mskew is not None else None
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    with gpu_meshes(c) as ms, contextlib.ExitStack() as stack:
        cams = stack.enter_context(Cameras(np.tile(c["K"].reshape(1, 9), (c["n"], 1)))) if table else None
        render_into(renderer, ms, c, frames.ptr, masks.ptr if masks else 0, stream.cuda_stream, cams)
        stream.synchronize()
        got_f = np.frombuffer(frames.read(), dtype=np.uint16).reshape(want_f.shape)
        got_m = np.frombuffer(masks.read(), dtype=np.uint8).reshape(want_m.shape) if masks else None
    clean = rr.resolve(rf.expected_keys(c))[0]
    assert not clean[-1].any() and clean[0].all()            # the empty frame is part of what must be written
    compare(got_f, got_m, c)


# ------------------------------------------------------------------ (c) renderer state
def test_first_call_drops_everything_then_the_deepest_lists():
    """A fresh renderer whose first call leaves the tile lists unallocated, then deep_lists on it."""
    none, deep = rf.all_cases()["all_dropped"], rf.all_cases()["deep_lists"]
    none["reach"](rf.census(none))
    with render.Renderer() as rd:
        with gpu_meshes(none) as ms:
            frames, masks = draw(rd, ms, none)
            assert frames.shape == (none["n"], none["h"], none["w"]) and not frames.any() and not masks.any()
            frames, masks = draw(rd, ms, none)
            assert not frames.any() and not masks.any()
        with gpu_meshes(deep) as ms:
            compare(*draw(rd, ms, deep), deep)


@pytest.mark.parametrize("label", ["deep_lists", "small_big_split"])
def test_twice_and_reversed_give_the_same_bytes(renderer, label):
    c = rf.all_cases()[label]
    with gpu_meshes(c) as ms:
        a = draw(renderer, ms, c)
        b = draw(renderer, ms, c)
        r = draw(renderer, ms, c, list(reversed(c["instances"])))
    compare(*a, c)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0].tobytes() == r[0].tobytes() and a[1].tobytes() == r[1].tobytes()
