"""The device-resident entry points at the edges of the caller's buffers.

The host entry points copy frames into the predictor's own aligned staging buffer and results out of its own workspace;
the `_device` calls read and write the caller's memory on the caller's stream.  Here every caller buffer sits inside a
larger torch allocation between two guard bands:

* outputs (mask, vote / blurred images, poses, decoded frames): >= 4 KB of seeded non-zero bytes on either side, and the
  output range itself pre-filled with the same pattern.  After the stream syncs the bands are unchanged and every byte of
  the output equals the reference (background mask pixels 0, every pose's `reserved` 0, a 2-D pose's rotation 0).
* inputs (frames, guesses, guess mask): bands of harmful values (65535 / random u16 around frames, NaN / huge values around
  guesses).  The output is byte-identical to the same call with zero bands, and to the oracle.

Outputs sit at skewed addresses (a mask at an odd byte, u16 images at 2 mod 4, poses at 8 mod 16), frames at 0 / 2 / 4 / 6
bytes past an 8-byte boundary with widths of every residue mod 4, so that both the 8-byte-load and the narrow-load paths
run.  Calls go to a non-default torch stream, each right behind an asynchronous upload of its frames on that stream.
Camera-table batches and tracker steps are held to the same bands: their `present` bytes between non-zero and zero bands.
"""
import os

import numpy as np
import pytest

from depthhead_amd import biwi, synth
from depthhead_amd._lib import POSE_DTYPE
from oracle import pyref

pytestmark = pytest.mark.gpu

GUARD = 4096
PB = POSE_DTYPE.itemsize


@pytest.fixture(scope="module")
def hp_mod(hip_lib):
    from depthhead_amd import prediction
    return prediction


@pytest.fixture(scope="module")
def torch_dev(hip_lib):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def aux_forest():
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 170, n_frames=12, subset=1500)
    assert (forest.leaf_prob >= 0.95).any()        # the vote image is not empty
    return forest


@pytest.fixture(scope="module")
def pose_forest():
    return synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)   # coherent votes: guesses matter


class env_at_creation:
    """Environment switches read when a predictor is created (DH_FORCE_GENERAL, DH_MAX_RESIDENT_FRAMES)."""

    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k in self.kv:
            os.environ.pop(k, None)


def _first_diff(a, b):
    d = np.flatnonzero(a != b)
    return f"{d.size} bytes differ, first at {d[0]}" if d.size else "equal"


class OutBuf:
    """`nbytes` of output at byte `skew` past a 256-byte boundary, between two bands of GUARD (+ skew) seeded non-zero
    bytes; the output range is pre-filled with the same pattern."""

    def __init__(self, torch_dev, nbytes, skew, seed):
        torch, dev = torch_dev
        self.torch = torch
        self.lo, self.n = GUARD + skew, nbytes
        self.init = np.random.default_rng(seed).integers(1, 256, self.lo + nbytes + GUARD, dtype=np.uint8)
        self.t = torch.from_numpy(self.init.copy()).to(dev)
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + self.lo

    def reset(self):
        self.t.copy_(self.torch.from_numpy(self.init))
        self.torch.cuda.synchronize()

    def result(self, what):
        """After the stream synced: the bands are intact; returns the output bytes."""
        got = self.t.cpu().numpy()
        lead, out, tail = got[: self.lo], got[self.lo: self.lo + self.n], got[self.lo + self.n:]
        assert np.array_equal(lead, self.init[: self.lo]), f"{what}: band in front written ({_first_diff(lead, self.init[: self.lo])})"
        assert np.array_equal(tail, self.init[self.lo + self.n:]), \
            f"{what}: band behind written ({_first_diff(tail, self.init[self.lo + self.n:])})"
        return out.copy()


def _harm_u16(nbytes, seed):
    g = np.random.default_rng(seed).integers(0, 65536, (nbytes + 1) // 2, dtype=np.uint16)
    g[::2] = 65535
    return g.view(np.uint8)[:nbytes]


def _harm_f32(nbytes, seed):
    g = np.random.default_rng(seed).uniform(-1e4, 1e4, (nbytes + 3) // 4).astype(np.float32)
    g[0::3], g[1::3] = np.nan, 3e38
    return g.view(np.uint8)[:nbytes]


def _harm_f64(nbytes, seed):
    g = np.random.default_rng(seed).uniform(-10.0, 10.0, (nbytes + 7) // 8)
    g[0::3], g[1::3] = np.nan, -1e300
    return g.view(np.uint8)[:nbytes]


def _harm_u8(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8) | np.uint8(3)   # every guess bit set


class InBuf:
    """An input of `nbytes` at byte `skew` past a 256-byte boundary between two bands made by `harm(nbytes, seed)` (or
    zeros with harm=None).  Before the data arrives the input range holds the harmful pattern too."""

    def __init__(self, torch_dev, nbytes, skew, seed, harm):
        torch, dev = torch_dev
        self.torch = torch
        self.lo, self.n = GUARD + skew, nbytes
        total = self.lo + nbytes + GUARD
        self.init = harm(total, seed) if harm else np.zeros(total, dtype=np.uint8)
        self.t = torch.from_numpy(self.init.copy()).to(dev)
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr() + self.lo
        self._keep = []

    def scramble(self):
        """The input range back to the band pattern (synchronously): a call that runs before its upload sees that."""
        self.t.copy_(self.torch.from_numpy(self.init))
        self.torch.cuda.synchronize()

    def upload(self, data, stream):
        """Asynchronous copy of `data` into the input range on `stream` (from page-locked memory, nothing waits)."""
        src = self.torch.from_numpy(np.ascontiguousarray(data).reshape(-1).view(np.uint8).copy()).pin_memory()
        assert src.numel() == self.n
        self._keep.append(src)
        with self.torch.cuda.stream(stream):
            self.t[self.lo: self.lo + self.n].copy_(src, non_blocking=True)

    def write(self, data):
        self.t[self.lo: self.lo + self.n].copy_(self.torch.from_numpy(np.ascontiguousarray(data).reshape(-1).view(np.uint8).copy()))

    def released(self):
        self._keep.clear()


def _poses_bytes(mid, rot):
    """The 40-byte records a pose output must hold: mid point, `reserved` 0, rotation."""
    out = np.zeros(len(mid), dtype=POSE_DTYPE)
    out["mid_point"], out["rotation"] = mid, rot
    return out.view(np.uint8)


def _aux_frames(n, w, h, first=80):
    frames = synth.biwi_batch(n, w, h, first=first)
    frames[2, : h // 2] = 0                        # half the frame background
    frames[3] = 0                                  # no vote at all: all-zero image, the last pixel wins the argmax
    frames[3, h - 1, w - 1] = 900
    return frames


def _aux_refs(oracle, forest, model, frames, K):
    mask = np.stack([oracle.predict_mask(forest, model, f) for f in frames])
    votes = np.stack([oracle.hough_image(forest, model, f, K) for f in frames])
    blurred = np.stack([oracle.build_hough_image(forest, model, f, K) for f in frames])
    p2 = [oracle.predict_from2dhough(forest, model, f, K) for f in frames]
    mid = np.stack([m for m, _ in p2])
    assert all(np.all(r == 0.0) for _, r in p2)
    return mask, votes, blurred, _poses_bytes(mid, np.zeros((len(frames), 3)))


AUX_KINDS = ("mask", "votes", "blurred", "poses2d")


def _aux_outs(torch_dev, n, w, h, seed):
    """Guard-banded outputs of the four aux calls: the mask at an odd byte, u16 images at 2 mod 4, poses at 8 mod 16."""
    return {"mask": OutBuf(torch_dev, n * w * h, 1, seed), "votes": OutBuf(torch_dev, n * w * h * 2, 2, seed + 1),
            "blurred": OutBuf(torch_dev, n * w * h * 2, 2, seed + 2), "poses2d": OutBuf(torch_dev, n * PB, 8, seed + 3)}


def _run_aux_device(hp, intr, fin, frames, outs, stream, scramble):
    """The four aux `_device` calls, each right behind an asynchronous upload of its frames on `stream`."""
    n, h, w = frames.shape
    calls = {"mask": lambda o: hp.predict_mask_device(fin.ptr, n, w, h, o, stream=stream.cuda_stream),
             "votes": lambda o: hp.hough_image_device(fin.ptr, n, w, h, intr, o, stream=stream.cuda_stream),
             "blurred": lambda o: hp.build_hough_image_device(fin.ptr, n, w, h, intr, o, stream=stream.cuda_stream),
             "poses2d": lambda o: hp.predict_from2dhough_device(fin.ptr, n, w, h, intr, o, stream=stream.cuda_stream)}
    got = {}
    for kind in AUX_KINDS:
        outs[kind].reset()
        if scramble:
            fin.scramble()
        fin.upload(frames, stream)
        calls[kind](outs[kind].ptr)
        stream.synchronize()
        got[kind] = outs[kind].result(kind)
    fin.released()
    return got


def _check_aux(got, refs, n, w, h, tag):
    mask, votes, blurred, poses = refs
    g = {"mask": got["mask"].reshape(n, h, w), "votes": got["votes"].view(np.uint16).reshape(n, h, w),
         "blurred": got["blurred"].view(np.uint16).reshape(n, h, w)}
    for i in range(n):
        assert np.array_equal(g["mask"][i], mask[i]), (tag, "mask", i, _first_diff(g["mask"][i], mask[i]))
        assert np.array_equal(g["votes"][i], votes[i]), (tag, "votes", i, _first_diff(g["votes"][i], votes[i]))
        assert np.array_equal(g["blurred"][i], blurred[i]), (tag, "blurred", i, _first_diff(g["blurred"][i], blurred[i]))
        assert np.array_equal(got["poses2d"][i * PB:(i + 1) * PB], poses[i * PB:(i + 1) * PB]), \
            (tag, "2-D pose record", i, got["poses2d"][i * PB:(i + 1) * PB], poses[i * PB:(i + 1) * PB])


# ------------------------------------------------------------------ (a) the four aux `_device` calls
@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("w,skew", [(200, 0), (200, 4), (201, 2), (202, 6), (203, 4)])
def test_aux_device_calls_inside_guard_bands(hp_mod, oracle, torch_dev, aux_forest, general, w, skew):
    """dh_predict_mask_device, dh_hough_image_device, dh_build_hough_image_device and dh_predict_from2dhough_device on
    frames at `skew` bytes past an 8-byte boundary (the 8-byte row loads need skew 0 and w % 4 == 0), outputs at skewed
    addresses between guard bands, on a non-default stream: byte for byte the oracle's, pyref's and the host twins' results;
    the same with zero bands around the frames."""
    torch, dev = torch_dev
    h, n = 150, 4
    model = synth.ModelParams(stepwidth=4, gaussian_sigma=2.5)
    frames = _aux_frames(n, w, h)
    K = synth.default_intrinsic(w, h)
    intr = hp_mod.IntrinsicMatrix(K)
    refs = _aux_refs(oracle, aux_forest, model, frames, K)
    assert refs[0].max() > 0 and refs[1].max() > 0 and refs[1][3].max() == 0
    assert refs[3].view(POSE_DTYPE)["mid_point"][3][2] == 900.0          # frame 3: the last pixel's depth
    for i in range(n):                                                     # the restatement's restatement agrees
        assert np.array_equal(pyref.predict_mask(aux_forest, model, frames[i]), refs[0][i]), (w, i)
        assert np.array_equal(pyref.hough_votes(aux_forest, model, frames[i], K)[0], refs[1][i]), (w, i)
    fbytes = n * w * h * 2
    harmful = InBuf(torch_dev, fbytes, skew, 11 + w, _harm_u16)
    zeros = InBuf(torch_dev, fbytes, skew, 0, None)
    outs = _aux_outs(torch_dev, n, w, h, 100 + w)
    st = torch.cuda.Stream(device=dev)
    with env_at_creation(DH_FORCE_GENERAL="1" if general else None):
        hp = hp_mod.HoughPrediction(aux_forest, model, device=0)
    with hp:
        hp.reserve(n, w, h)
        assert hp.debug_geometry()["uniform"] == 0 or not general
        torch.cuda.synchronize()
        # zero bands first (this also makes the aux scratch and the blur taps, with their device-wide syncs), then the
        # harmful bands with every call right behind its upload and nothing in between
        plain = _run_aux_device(hp, intr, zeros, frames, outs, st, scramble=False)
        got = _run_aux_device(hp, intr, harmful, frames, outs, st, scramble=True)
        host = {"mask": hp.predict_mask(frames).reshape(-1), "votes": hp.build_hough_votes(frames, intr).reshape(-1).view(np.uint8),
                "blurred": hp.build_hough_image(frames, intr).reshape(-1).view(np.uint8),
                "poses2d": hp.predict_parameter_from2dhough(frames, intr).view(np.uint8)}
    tag = (w, skew, general)
    _check_aux(got, refs, n, w, h, tag)
    for kind in AUX_KINDS:
        assert np.array_equal(got[kind], plain[kind]), (tag, kind, "harmful vs zero bands", _first_diff(got[kind], plain[kind]))
        assert np.array_equal(got[kind], host[kind]), (tag, kind, "device vs host twin", _first_diff(got[kind], host[kind]))


# ------------------------------------------------------------------ (b) predict_batch_device and decode_depth_device
def _pose_refs(oracle, forest, model, frames, K, mg=None, rg=None, gm=None):
    """Oracle poses frame by frame: the guess mask decides whether a frame's guess is passed or None."""
    n = len(frames)
    gm = np.full(n, 3, dtype=np.uint8) if gm is None else gm
    mid, rot = np.zeros((n, 3), dtype=np.float32), np.zeros((n, 3))
    for k in range(4):
        s = gm == k
        if s.any():
            r = oracle.predict_batch(forest, model, frames[s], K, mg[s] if mg is not None and k & 1 else None,
                                     rg[s] if rg is not None and k & 2 else None)
            mid[s], rot[s] = r["mid_point"], r["rotation"]
    return _poses_bytes(mid, rot)


def _check_poses(got, ref, tag):
    n = ref.size // PB
    for i in range(n):
        g, r = got[i * PB:(i + 1) * PB], ref[i * PB:(i + 1) * PB]
        assert np.array_equal(g, r), (tag, "frame", i, g.view(POSE_DTYPE), r.view(POSE_DTYPE))


@pytest.mark.parametrize("chunks", [1, 2, 3])
def test_predict_batch_device_inside_guard_bands(hp_mod, oracle, torch_dev, pose_forest, chunks):
    """Product-mode device batches, unforked and forked into 2 / 3 sub-batches (50 frames: 25 / 25 and 16 / 17 / 17):
    every 40-byte record written (the pattern under them included), the bands around the poses intact, the frames at a
    2 mod 4 address between harmful bands, the result the same as with zero bands."""
    torch, dev = torch_dev
    w, h, n = 202, 152, 50
    model = synth.ModelParams(stepwidth=4)
    frames = synth.biwi_batch(n, w, h, first=200)
    frames[7] = 0
    K = synth.default_intrinsic(w, h)
    intr = hp_mod.IntrinsicMatrix(K)
    ref = _pose_refs(oracle, pose_forest, model, frames, K)
    harmful = InBuf(torch_dev, frames.nbytes, 2, 5, _harm_u16)
    zeros = InBuf(torch_dev, frames.nbytes, 2, 0, None)
    out = OutBuf(torch_dev, n * PB, 8, 40 + chunks)
    st = torch.cuda.Stream(device=dev)
    with hp_mod.HoughPrediction(pose_forest, model, device=0) as hp:
        hp.set_forking(chunks)
        hp.reserve(n, w, h)
        for fin in (harmful, zeros):
            out.reset()
            fin.scramble()
            fin.upload(frames, st)
            hp.predict_batch_device(fin.ptr, n, w, h, intr, out.ptr, stream=st.cuda_stream)
            st.synchronize()
            fin.released()
            _check_poses(out.result("poses"), ref, ("chunks", chunks, "zero bands" if fin is zeros else "harmful bands"))


def test_decode_depth_device_fills_exactly_its_frames(hp_mod, torch_dev, pose_forest):
    """dh_biwi_decode_depth_device into a caller buffer of exactly n*w*h pixels at a 2 mod 4 address: every pixel (the
    zero runs too, over the non-zero pattern) written, the bands in front of the first and behind the last frame intact."""
    w, h, n = 203, 151, 5
    frames = synth.biwi_batch(n, w, h, first=300)
    frames[1] = 0
    frames[2, :, ::3] = 0
    payloads = [biwi.encode_depth(f) for f in frames]
    out = OutBuf(torch_dev, frames.nbytes, 2, 77)
    with hp_mod.HoughPrediction(pose_forest, synth.ModelParams(stepwidth=4), device=0) as hp:
        assert hp.decode_depth_device(payloads, out.ptr, n * w * h) == (w, h)
    got = out.result("decoded frames").view(np.uint16).reshape(n, h, w)
    for i in range(n):
        assert np.array_equal(got[i], frames[i]), (i, _first_diff(got[i], frames[i]))


# ------------------------------------------------------------------ (c) guesses held in device memory
def _guesses(base, n):
    """Per-frame guesses that all differ: near each frame's pose, moved by a different amount per frame; mask 0, 1, 2, 3."""
    i = np.arange(n)
    pose = base.view(POSE_DTYPE)
    mg = (pose["mid_point"] + np.stack([3.0 + 0.7 * i, -2.0 - 0.5 * (i % 7), 4.0 + 1.1 * (i % 5)], 1)).astype(np.float32)
    rg = pose["rotation"] + 0.03 + 0.011 * (i % 9)[:, None]
    gm = (i % 4).astype(np.uint8)
    return mg, rg, gm


class GuessBufs:
    """midp (f32, 4 mod 8), rot (f64, 8 mod 16) and mask (odd byte) between bands of NaN / huge values, or zeros."""

    def __init__(self, torch_dev, n, seed, harmful=True):
        self.mg = InBuf(torch_dev, n * 12, 4, seed, _harm_f32 if harmful else None)
        self.rg = InBuf(torch_dev, n * 24, 8, seed + 1, _harm_f64 if harmful else None)
        self.gm = InBuf(torch_dev, n, 1, seed + 2, _harm_u8 if harmful else None)

    def upload(self, mg, rg, gm, stream):
        for b, d in ((self.mg, mg), (self.rg, rg), (self.gm, gm)):
            b.upload(d, stream)

    def write(self, mg, rg, gm):
        for b, d in ((self.mg, mg), (self.rg, rg), (self.gm, gm)):
            b.write(d)

    def released(self):
        for b in (self.mg, self.rg, self.gm):
            b.released()


def _guess_case(oracle, forest, model, n, w, h, first):
    frames = synth.biwi_batch(n, w, h, first=first)
    K = synth.default_intrinsic(w, h)
    base = _pose_refs(oracle, forest, model, frames, K)
    mg, rg, gm = _guesses(base, n)
    ref = _pose_refs(oracle, forest, model, frames, K, mg, rg, gm)
    # a guess read at the wrong frame offset changes the result: the same with the guesses moved by one frame differs
    shifted = _pose_refs(oracle, forest, model, frames, K, np.roll(mg, 1, 0), np.roll(rg, 1, 0), gm)
    differ = [i for i in range(n) if not np.array_equal(ref[i * PB:(i + 1) * PB], shifted[i * PB:(i + 1) * PB])]
    assert differ, "guesses moved by one frame give the same poses: the test could not see a misplaced guess"
    assert not np.array_equal(ref, base)
    return frames, K, mg, rg, gm, ref


@pytest.mark.parametrize("chunks,n,resident", [(1, 50, None), (2, 50, None), (3, 50, None), (1, 11, "4")])
def test_device_resident_guesses(hp_mod, oracle, torch_dev, pose_forest, chunks, n, resident):
    """midp_guess / rot_guess / guess_mask as device pointers inside guard bands: unforked, forked into 2 and 3 sub-batches
    (50 frames: 25 / 25, 16 / 17 / 17), and beyond the resident slice (4 frames resident, 11 frames); every pose against
    the oracle run with the frame's own guesses, the result the same with zero bands around every input."""
    torch, dev = torch_dev
    w, h = 201, 150
    model = synth.ModelParams(stepwidth=4)
    frames, K, mg, rg, gm, ref = _guess_case(oracle, pose_forest, model, n, w, h, 400)
    intr = hp_mod.IntrinsicMatrix(K)
    st = torch.cuda.Stream(device=dev)
    out = OutBuf(torch_dev, n * PB, 8, 60 + chunks)
    with env_at_creation(DH_MAX_RESIDENT_FRAMES=resident):
        hp = hp_mod.HoughPrediction(pose_forest, model, device=0)
    with hp:
        hp.set_forking(chunks)
        hp.reserve(n, w, h)
        for harmful in (True, False):
            fin = InBuf(torch_dev, frames.nbytes, 2, 9, _harm_u16 if harmful else None)
            gb = GuessBufs(torch_dev, n, 20, harmful)
            out.reset()
            fin.upload(frames, st)
            gb.upload(mg, rg, gm, st)
            hp.predict_batch_device(fin.ptr, n, w, h, intr, out.ptr, gb.mg.ptr, gb.rg.ptr, gb.gm.ptr, stream=st.cuda_stream)
            st.synchronize()
            fin.released()
            gb.released()
            _check_poses(out.result("poses"), ref, (chunks, n, resident, "harmful" if harmful else "zero", "bands"))


@pytest.mark.parametrize("resident", [None, "4"])
def test_graph_replays_with_device_guesses_rewritten_in_place(hp_mod, oracle, torch_dev, pose_forest, resident):
    """dh_graph_capture with guess pointers inside guard bands; frames, guesses and mask rewritten in place between
    replays (the captured pointers stay), every replay against the oracle.  Also captured over resident slices."""
    torch, dev = torch_dev
    w, h, n = 200, 150, 11
    model = synth.ModelParams(stepwidth=4)
    cases = [_guess_case(oracle, pose_forest, model, n, w, h, first) for first in (500, 520, 540)]
    K = cases[0][1]
    intr = hp_mod.IntrinsicMatrix(K)
    fin = InBuf(torch_dev, cases[0][0].nbytes, 6, 3, _harm_u16)
    gb = GuessBufs(torch_dev, n, 30)
    out = OutBuf(torch_dev, n * PB, 8, 90)
    st = torch.cuda.current_stream(dev)
    with env_at_creation(DH_MAX_RESIDENT_FRAMES=resident):
        hp = hp_mod.HoughPrediction(pose_forest, model, device=0)
    with hp:
        hp.reserve(n, w, h)
        hp.graph_capture(fin.ptr, n, w, h, intr, out.ptr, gb.mg.ptr, gb.rg.ptr, gb.gm.ptr)
        for rep, k in enumerate((0, 1, 2, 0)):
            frames, _, mg, rg, gm, ref = cases[k]
            out.reset()
            fin.write(frames)
            gb.write(mg, rg, gm)
            hp.graph_launch(st.cuda_stream)
            st.synchronize()
            _check_poses(out.result("poses"), ref, ("replay", rep, "case", k, resident))


# ------------------------------------------------------------------ (d) slices on the aux path
def test_aux_calls_beyond_the_resident_slice(hp_mod, oracle, torch_dev, aux_forest):
    """4 frames resident, 11 frames: the four host aux calls and the four `_device` calls walk three slices; every frame
    of every output against the oracle (the 2-D poses from from2dhough), the device outputs inside guard bands."""
    torch, dev = torch_dev
    w, h, n = 201, 150, 11
    model = synth.ModelParams(stepwidth=4, gaussian_sigma=2.5)
    frames = np.concatenate([_aux_frames(4, w, h, first=80), synth.biwi_batch(n - 4, w, h, first=600)])
    frames[9] = frames[3]                                    # a no-vote frame inside the last slice as well
    K = synth.default_intrinsic(w, h)
    intr = hp_mod.IntrinsicMatrix(K)
    refs = _aux_refs(oracle, aux_forest, model, frames, K)
    fin = InBuf(torch_dev, frames.nbytes, 2, 13, _harm_u16)
    outs = _aux_outs(torch_dev, n, w, h, 700)
    st = torch.cuda.Stream(device=dev)
    with env_at_creation(DH_MAX_RESIDENT_FRAMES="4"):
        hp = hp_mod.HoughPrediction(aux_forest, model, device=0)
    with hp:
        host = {"mask": hp.predict_mask(frames).reshape(-1), "votes": hp.build_hough_votes(frames, intr).reshape(-1).view(np.uint8),
                "blurred": hp.build_hough_image(frames, intr).reshape(-1).view(np.uint8),
                "poses2d": hp.predict_parameter_from2dhough(frames, intr).view(np.uint8)}
        torch.cuda.synchronize()
        got = _run_aux_device(hp, intr, fin, frames, outs, st, scramble=True)
    _check_aux(host, refs, n, w, h, "host, 4 resident")
    _check_aux(got, refs, n, w, h, "device, 4 resident")


# ------------------------------------------------------------------ (e) aux calls between product batches
def test_aux_device_calls_between_product_batches(hp_mod, oracle, torch_dev, aux_forest):
    """One predictor: the four aux `_device` calls interleaved with 280 product-mode device batches -- past the wrap of the
    255-value tile-flag tag -- some of them forked in 2 or 3; every output against precomputed oracle results."""
    torch, dev = torch_dev
    w, h, nf = 200, 150, 48
    model = synth.ModelParams(stepwidth=4, gaussian_sigma=2.5)
    K = synth.default_intrinsic(w, h)
    intr = hp_mod.IntrinsicMatrix(K)
    base = synth.biwi_batch(3, w, h, first=40)
    pool = np.stack([base[0], np.roll(base[1], 60, axis=1), np.zeros((h, w), dtype=np.uint16), np.roll(base[2], -50, axis=1)])
    pool_ref = _pose_refs(oracle, aux_forest, model, pool, K)
    fork_idx = (np.arange(nf) * 5 + np.arange(nf) // 3) % 4
    fork_ref = np.concatenate([pool_ref[k * PB:(k + 1) * PB] for k in fork_idx])
    aux_frames = _aux_frames(4, w, h)
    aux_refs = _aux_refs(oracle, aux_forest, model, aux_frames, K)
    one_in, one_out = InBuf(torch_dev, w * h * 2, 2, 17, _harm_u16), OutBuf(torch_dev, PB, 8, 800)
    many_in, many_out = InBuf(torch_dev, nf * w * h * 2, 6, 18, _harm_u16), OutBuf(torch_dev, nf * PB, 8, 801)
    aux_in = InBuf(torch_dev, aux_frames.nbytes, 4, 19, _harm_u16)
    outs = _aux_outs(torch_dev, 4, w, h, 900)
    st = torch.cuda.Stream(device=dev)
    with hp_mod.HoughPrediction(aux_forest, model, device=0) as hp:
        hp.reserve(nf, w, h)
        torch.cuda.synchronize()
        for i in range(280):
            if i % 40 == 39:
                got = _run_aux_device(hp, intr, aux_in, aux_frames, outs, st, scramble=False)
                _check_aux(got, aux_refs, 4, w, h, ("aux after batch", i))
            forked = i % 25 == 12
            if forked:
                hp.set_forking(2 if i % 50 == 12 else 3)
                fin, out, frames, ref = many_in, many_out, pool[fork_idx], fork_ref
            else:
                k = (i * 7 + i // 5) % 4
                fin, out, frames, ref = one_in, one_out, pool[k:k + 1], pool_ref[k * PB:(k + 1) * PB]
            out.reset()
            fin.upload(frames, st)
            hp.predict_batch_device(fin.ptr, len(frames), w, h, intr, out.ptr, stream=st.cuda_stream)
            st.synchronize()
            fin.released()
            _check_poses(out.result("poses"), ref, ("batch", i, "forked" if forked else "whole"))
            if forked:
                hp.set_forking(0)


# ------------------------------------------------------------------ (d) camera tables and tracker steps on device buffers
@pytest.mark.parametrize("chunks", [1, 2, 3])
def test_predict_batch_cameras_device_inside_guard_bands(hp_mod, oracle, torch_dev, pose_forest, chunks):
    """dh_predict_batch_cameras_device, unforked and forked into 2 / 3 sub-batches: frames at 2 mod 4, guesses and the guess
    mask between harmful bands, poses at 8 mod 16 on a non-default stream; every record written, the bands intact, frame i
    the oracle's with camera i's K and its own guesses, byte-identical with zero bands around every input."""
    from depthhead_amd.tracking import Cameras
    from test_gpu_tracking import cameras_k
    torch, dev = torch_dev
    w, h, n = 202, 152, 50
    model = synth.ModelParams(stepwidth=4)
    Ks = cameras_k(w, h)
    cam_of = (np.arange(n) * 3) % len(Ks)
    frames = synth.biwi_batch(n, w, h, first=600)
    base = np.zeros(n * PB, dtype=np.uint8)
    for c in range(len(Ks)):
        idx = np.flatnonzero(cam_of == c)
        base.reshape(n, PB)[idx] = _pose_refs(oracle, pose_forest, model, frames[idx], Ks[c]).reshape(-1, PB)
    mg, rg, gm = _guesses(base, n)
    ref = np.zeros(n * PB, dtype=np.uint8)
    for c in range(len(Ks)):
        idx = np.flatnonzero(cam_of == c)
        ref.reshape(n, PB)[idx] = _pose_refs(oracle, pose_forest, model, frames[idx], Ks[c], mg[idx], rg[idx], gm[idx]).reshape(-1, PB)
    st = torch.cuda.Stream(device=dev)
    out = OutBuf(torch_dev, n * PB, 8, 80 + chunks)
    got = []
    with hp_mod.HoughPrediction(pose_forest, model, device=0) as hp, Cameras(Ks[cam_of]) as cams:
        hp.set_forking(chunks)
        hp.reserve(n, w, h)
        for harmful in (True, False):
            fin = InBuf(torch_dev, frames.nbytes, 2, 13, _harm_u16 if harmful else None)
            gb = GuessBufs(torch_dev, n, 30, harmful)
            out.reset()
            fin.upload(frames, st)
            gb.upload(mg, rg, gm, st)
            hp.predict_batch_cameras_device(fin.ptr, n, w, h, cams, out.ptr, gb.mg.ptr, gb.rg.ptr, gb.gm.ptr, stream=st.cuda_stream)
            st.synchronize()
            fin.released()
            gb.released()
            got.append(out.result("poses"))
            _check_poses(got[-1], ref, (chunks, "harmful" if harmful else "zero", "bands"))
    assert got[0].tobytes() == got[1].tobytes()


def test_tracker_step_device_inside_guard_bands(hp_mod, oracle, torch_dev):
    """dh_tracker_step_device on a non-default stream: the `present` bytes between bands of non-zero bytes (and of zero
    bytes), frames between harmful bands, poses at 8 mod 16 between guard bands.  Every step's records equal the live-loop
    restatement and the zero-band run byte for byte; the bands stay intact; the final tracker states are identical."""
    from depthhead_amd.tracking import Cameras, HeadTracker
    from test_gpu_tracking import RESET_AT, RESET_CAM, STEPS, live_loop_restatement, present_at, track_frames
    torch, dev = torch_dev
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)
    model = synth.ModelParams(stepwidth=4)
    Ks, frames = track_frames()
    C, h, w = frames.shape[1], frames.shape[2], frames.shape[3]
    ref_poses, _, _, _ = live_loop_restatement(oracle, forest, model, Ks, frames, True, False)
    st = torch.cuda.Stream(device=dev)
    runs = []
    for harmful in (True, False):
        out = OutBuf(torch_dev, C * PB, 8, 90)
        fin = InBuf(torch_dev, frames[0].nbytes, 2, 17, _harm_u16 if harmful else None)
        pin = InBuf(torch_dev, C, 1, 19, _harm_u8 if harmful else None)
        steps = []
        with hp_mod.HoughPrediction(forest, model, device=0) as hp, Cameras(Ks) as cams, \
                HeadTracker(hp, cams, w, h, prev_guess=True, sluggish=False) as tr:
            for t in range(STEPS):
                if t == RESET_AT:
                    tr.reset(RESET_CAM, stream=st.cuda_stream)
                out.reset()
                fin.upload(frames[t], st)
                pin.upload(present_at(t, C), st)
                tr.step_device(fin.ptr, out.ptr, pin.ptr, stream=st.cuda_stream)
                st.synchronize()
                fin.released()
                pin.released()
                got = out.result(f"poses of step {t}")
                want = _poses_bytes(np.stack([m for m, _ in ref_poses[t]]), np.stack([r for _, r in ref_poses[t]]))
                _check_poses(got, want, (t, "harmful" if harmful else "zero", "bands"))
                steps.append(got)
            runs.append((steps, tr.state()))
    (a, sa), (b, sb) = runs
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for k in ("midp", "rot", "mask", "has_rot"):
        assert sa[k].tobytes() == sb[k].tobytes(), k
