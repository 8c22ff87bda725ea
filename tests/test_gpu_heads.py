"""Several heads per frame on the GPU (dh_predict_heads and its camera / device twins), byte for byte against the CPU
restatement of tests/heads_ref.py:

* both traversal paths (uniform box sums; DH_FORCE_GENERAL=1), strides 3 - 5, frames 128 x 112 .. 640 x 480, max_heads 1 - 4;
* batches of 1, 7 and 256 frames, host and device calls, forked sub-batches, a mixed-camera table, resident slices of 3
  frames (a child process with DH_MAX_RESIDENT_FRAMES=3);
* predict_batch's bytes in the same workspace do not change around a heads call, and at radius 2^31 - 1 every head's rotation
  is the plain call's where every rotation-voting hit also casts a position vote.
Frames are two stream frames composited (the nearer non-zero pixel), so that they hold two heads; every test asserts that its
frames reach a frame with two heads and a seed merged into another head.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from depthhead_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_ref as hr  # noqa: E402
import support_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOREST_ARGS = (6, 10, synth.FOREST_SEED_BASE + 9)


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import _lib, prediction, tracking
    return _lib, prediction, tracking


@pytest.fixture(scope="module")
def forest():
    return synth.fit_forest(*FOREST_ARGS, n_frames=12, subset=1500)


@pytest.fixture(scope="module")
def tables(forest):
    return sr.LeafTables(forest)


# A stream frame whose seeds reach one mode (a seed merged into another head) at each (w, h, stride) the tests use: merging needs
# two seeds three guess cells apart to end within 20 mm, which few frames do.
MERGE_FRAME = {(128, 112, 4): 63, (128, 112, 3): 86, (320, 240, 5): 1, (640, 480, 5): 121}


def two_head_frames(n, w, h, first=0, stride=4):
    """Frame i: stream frame first + i beside stream frame first + 500 + i moved by a third of the width; the last frame is
    MERGE_FRAME's."""
    a = synth.biwi_batch(n, w, h, first=first)
    b = synth.biwi_batch(n, w, h, first=first + 500)
    out = np.empty_like(a)
    s = w // 3
    for i in range(n):
        moved = np.zeros_like(b[i])
        if i % 2:
            moved[:, s:] = b[i][:, : w - s]
        else:
            moved[:, : w - s] = b[i][:, s:]
        out[i] = hr.composite(a[i], moved)
    if n > 2:
        out[1] = 0                                      # an empty frame: no heads
    out[n - 1] = synth.biwi_batch(1, w, h, first=MERGE_FRAME[(w, h, stride)])[0]
    return out


def expect(oracle, tables, model, frames, Ks, max_heads, radius):
    """(n_heads, HEAD_DTYPE [n, max_heads], two-head frames, merged seeds) of a batch; Ks: one K or one per frame."""
    from depthhead_amd._lib import HEAD_DTYPE
    n = frames.shape[0]
    nh = np.zeros(n, np.uint32)
    recs = np.zeros((n, max_heads), dtype=HEAD_DTYPE)
    two = merged = 0
    for i in range(n):
        K = Ks[i] if np.ndim(Ks) == 3 else Ks
        k, kept, info, _, _ = hr.heads_ref(oracle, tables, model, frames[i], K, max_heads, radius)
        nh[i] = k
        recs[i] = hr.as_records(k, kept, max_heads, HEAD_DTYPE)
        two += k >= 2
        merged += info["merged"]
    return nh, recs, two, merged


def assert_heads(got_n, got, want_n, want, what):
    assert np.array_equal(got_n, want_n), (what, got_n, want_n)
    for i in range(len(want_n)):
        assert got[i].tobytes() == want[i].tobytes(), (what, i, got[i], want[i])


def coverage(two, merged, what):
    assert two >= 1, f"{what}: no frame with two heads"
    assert merged >= 1, f"{what}: no seed merged into another head"


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("stride,w,h,radius,first", [(4, 128, 112, 30, 0), (3, 128, 112, 20, 3), (5, 320, 240, 40, 5),
                                                     (5, 640, 480, 30, 8)])
def test_heads_match_restatement(mods, forest, tables, oracle, monkeypatch, general, stride, w, h, radius, first):
    _lib, prediction, _ = mods
    if general:
        monkeypatch.setenv("DH_FORCE_GENERAL", "1")
    model = synth.ModelParams(stepwidth=stride)
    K = synth.default_intrinsic(w, h)
    n = 3 if w >= 640 else 7
    frames = two_head_frames(n, w, h, first=first, stride=stride)
    two = merged = 0
    with prediction.HoughPrediction(forest, model) as hp:
        for mh in (4, 3, 2, 1):
            want_n, want, t, m = expect(oracle, tables, model, frames, K, mh, radius)
            two += t if mh > 1 else 0
            merged += m
            got_n, got = hp.predict_heads(frames, prediction.IntrinsicMatrix(K), mh, radius)
            if general:
                assert hp.debug_geometry()["uniform"] == 0
            assert_heads(got_n, got, want_n, want, f"host batch of {n}, max_heads {mh}")
            again_n, again = hp.predict_heads(frames, prediction.IntrinsicMatrix(K), mh, radius)
            assert again.tobytes() == got.tobytes() and again_n.tobytes() == got_n.tobytes()
            one_n, one = hp.predict_heads(frames[2:3], prediction.IntrinsicMatrix(K), mh, radius)
            assert_heads(one_n, one, want_n[2:3], want[2:3], "batch of 1")
            assert got_n[1] == 0 and got[1].tobytes() == bytes(got[1].nbytes)
    coverage(two, merged, f"{w}x{h} stride {stride}")


def test_heads_256_device_forked_and_plain_unchanged(mods, forest, tables, oracle):
    """256 frames (16 distinct, repeated) through the device call, whole and as forked sub-batches; predict_batch's bytes in the
    same workspace are the same before and after."""
    import torch
    _lib, prediction, _ = mods
    w, h = 128, 112
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(w, h)
    base = two_head_frames(16, w, h, first=20)
    want_n16, want16, two, merged = expect(oracle, tables, model, base, K, 4, 30)
    coverage(two, merged, "256 frames")
    idx = np.arange(256) % 16
    frames = base[idx]
    dev = torch.device("cuda", 0)
    ft = torch.from_numpy(frames).to(dev)
    with prediction.HoughPrediction(forest, model) as hp:
        plain0 = hp.predict_batch(frames, prediction.IntrinsicMatrix(K))
        for chunks in (1, 2):
            hp.set_forking(chunks)
            nd = torch.zeros(256, dtype=torch.int32, device=dev)
            hd = torch.zeros(256 * 4 * 80, dtype=torch.uint8, device=dev)
            hp.predict_heads_device(ft.data_ptr(), 256, w, h, prediction.IntrinsicMatrix(K), nd.data_ptr(), hd.data_ptr(), 4, 30,
                                    stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got_n = nd.cpu().numpy().view(np.uint32)
            got = hd.cpu().numpy().view(_lib.HEAD_DTYPE).reshape(256, 4)
            assert_heads(got_n, got, want_n16[idx], want16[idx], f"device batch of 256, {chunks} chunk(s)")
        hp.set_forking(0)
        plain1 = hp.predict_batch(frames, prediction.IntrinsicMatrix(K))
        host_n, host = hp.predict_heads(frames, prediction.IntrinsicMatrix(K), 4, 30)
        assert_heads(host_n, host, want_n16[idx], want16[idx], "host batch of 256")
    assert plain0.tobytes() == plain1.tobytes()


def cameras_k(n=7, w=128, h=112):
    K0 = synth.default_intrinsic(w, h).astype(np.float32)
    Ks = np.repeat(K0[None], n, axis=0)
    for i in range(1, n, 2):
        Ks[i, 0, 0] *= 1.1 + 0.05 * i
        Ks[i, 1, 1] *= 1.1 + 0.05 * i
        Ks[i, 0, 2] += 3 * i
    Ks[n - 1, 0, 1] = 0.5                              # one camera that is not pinhole
    return Ks


def test_heads_mixed_cameras_host_and_device(mods, forest, tables, oracle):
    import torch
    _lib, prediction, tracking = mods
    w, h = 128, 112
    model = synth.ModelParams(stepwidth=4)
    Ks = cameras_k()
    n = len(Ks)
    frames = two_head_frames(n, w, h, first=30)
    want_n, want, two, merged = expect(oracle, tables, model, frames, Ks, 4, 30)
    coverage(two, merged, "mixed cameras")
    dev = torch.device("cuda", 0)
    with prediction.HoughPrediction(forest, model) as hp, tracking.Cameras(Ks) as cams:
        got_n, got = hp.predict_heads_cameras(frames, cams, 4, 30)
        assert_heads(got_n, got, want_n, want, "camera host batch")
        ft = torch.from_numpy(frames).to(dev)
        nd = torch.zeros(n, dtype=torch.int32, device=dev)
        hd = torch.zeros(n * 3 * 80, dtype=torch.uint8, device=dev)
        hp.predict_heads_cameras_device(ft.data_ptr(), n, w, h, cams, nd.data_ptr(), hd.data_ptr(), 3, 30,
                                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want_n3, want3, _, _ = expect(oracle, tables, model, frames, Ks, 3, 30)
        assert_heads(nd.cpu().numpy().view(np.uint32), hd.cpu().numpy().view(_lib.HEAD_DTYPE).reshape(n, 3), want_n3, want3,
                     "camera device batch")


def test_heads_across_resident_slices(mods, forest, tables, oracle, tmp_path):
    """DH_MAX_RESIDENT_FRAMES = 3 in a fresh child process: slices offset the heads and the cameras as they offset poses."""
    _lib = mods[0]
    w, h = 128, 112
    model = synth.ModelParams(stepwidth=4)
    Ks = cameras_k()
    n = len(Ks)
    frames = two_head_frames(n, w, h, first=60)
    K = synth.default_intrinsic(w, h)
    np.savez(str(tmp_path / "in.npz"), frames=frames, Ks=Ks, K=K)
    code = (
        "import numpy as np, sys, json\n"
        "from depthhead_amd import synth\n"
        "from depthhead_amd.prediction import HoughPrediction, IntrinsicMatrix\n"
        "from depthhead_amd.tracking import Cameras\n"
        "d = np.load(sys.argv[1])\n"
        f"forest = synth.fit_forest({FOREST_ARGS[0]}, {FOREST_ARGS[1]}, {FOREST_ARGS[2]}, n_frames=12, subset=1500)\n"
        "with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, Cameras(d['Ks']) as cams:\n"
        "    a, b = hp.predict_heads_cameras(d['frames'], cams, 4, 30)\n"
        "    c, e = hp.predict_heads(d['frames'], IntrinsicMatrix(d['K']), 2, 30)\n"
        "print(json.dumps({k: v.tobytes().hex() for k, v in dict(a=a, b=b, c=c, e=e).items()}))\n")
    env = dict(os.environ, DH_MAX_RESIDENT_FRAMES="3")
    res = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz")], capture_output=True, text=True, env=env,
                         cwd=ROOT, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    want_n, want, two, merged = expect(oracle, tables, model, frames, Ks, 4, 30)
    coverage(two, merged, "camera slices of 3")
    assert_heads(np.frombuffer(bytes.fromhex(got["a"]), np.uint32), np.frombuffer(bytes.fromhex(got["b"]), _lib.HEAD_DTYPE).reshape(n, 4),
                 want_n, want, "camera slices of 3")
    want_n2, want2, _, _ = expect(oracle, tables, model, frames, K, 2, 30)
    assert_heads(np.frombuffer(bytes.fromhex(got["c"]), np.uint32), np.frombuffer(bytes.fromhex(got["e"]), _lib.HEAD_DTYPE).reshape(n, 2),
                 want_n2, want2, "slices of 3")


def test_full_radius_rotation_is_the_plain_rotation(mods, forest, tables, oracle):
    """At r = 2^31 - 1 every hit with a position vote supports every head: where every rotation-voting hit of the frame also
    casts a position vote, each head's rotation is the plain call's, bit for bit."""
    _lib, prediction, _ = mods
    w, h = 128, 112
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(w, h)
    frames = two_head_frames(7, w, h, first=90)
    full = (1 << 31) - 1
    want_n, want, two, merged = expect(oracle, tables, model, frames, K, 4, full)
    coverage(two, 1, "full radius")                    # (merging does not depend on the radius)
    with prediction.HoughPrediction(forest, model) as hp:
        plain = hp.predict_batch(frames, prediction.IntrinsicMatrix(K))
        got_n, got = hp.predict_heads(frames, prediction.IntrinsicMatrix(K), 4, full)
    assert_heads(got_n, got, want_n, want, "radius 2^31 - 1")
    same = 0
    for i in range(len(frames)):
        res = oracle.predict(forest, model, frames[i], K, taps=True)
        fh = hr.frame_hits(tables, model, frames[i], K, res.leaf_idx, res.patch_flags)
        c, v = hr.accumulate(fh["rot_cells"], fh["rot_vals"])
        rc = res.rot_cells.astype(np.int64)
        if not (len(c) == len(rc) and np.array_equal(c, rc[:, :3]) and np.array_equal(v, rc[:, 3] % (1 << 32))):
            continue                                   # some rotation-voting hit casts no position vote
        for j in range(int(got_n[i])):
            assert got[i, j]["pose"]["rotation"].tobytes() == plain[i]["rotation"].tobytes(), (i, j)
            same += 1
    assert same >= 3, same
