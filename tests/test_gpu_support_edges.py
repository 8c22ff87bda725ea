"""Vote support (k_emit's SUP instances, k_support) at its edges, byte for byte against the restatement of
tests/support_ref.py:

(a) every one of the 20 `k_emit<EB, LS, CAM, SUP = true>` instances: forests of 3 .. 70 trees (EB 4 / 8 / 10 / 12 / 16, the
    multi-batch gather, the generic hit search above 64 trees) with 2-byte and 4-byte window-list entries (LS 1 / 2), through
    a single-K batch (CAM = false) and a mixed pinhole / general camera table (CAM = true);
(b) the adversarial families of tests/edge_families.py on both traversal paths, through single-K batches and decoy-camera
    tables, at radii 0, DH_SUPPORT_RADIUS, 2^31 - 1 and a boundary pair r*, r* - 1, judged by the pyref-sourced restatement
    (tests/test_support_families.py), and the reach of the whole parametrization on the kernels' own records;
(c) k_support's launch shapes: a few hundred workgroups on one 640 x 480 frame, a grid-stride loop of several passes
    (512 frames), one workgroup per frame (2048 frames in one launch, in a child process);
(d) the support scratch's lifecycle on one predictor, and the first support call after a graph capture;
(e) the three `_device` support calls between guard bands, unforked and forked.
Poses of every support call are byte-identical to the plain call's.
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_families as ef
import support_ref as sr
from depthhead_amd import synth
from test_gpu_device_buffers import InBuf, OutBuf, _harm_f32, _harm_u16, _harm_u8
from test_gpu_edge_families import REFUSED, general_path
from test_gpu_support import assert_support, cameras_k, expect, frames_for
from test_support_families import Reach, family_support

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SB = 40                     # sizeof(dh_support) == sizeof(dh_pose)
SUP_THREADS = 256           # k_support.hip


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import _lib, prediction, tracking
    return _lib, prediction, tracking


@pytest.fixture(scope="module")
def torch_dev(hip_lib):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def pose_forest():
    return synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)   # coherent votes (smoke())


@pytest.fixture(scope="module")
def pose_tables(pose_forest):
    return sr.LeafTables(pose_forest)


def support_grid_x(n_frames, hits_cap):
    """Workgroups per frame of dh_launch_support (k_support.hip)."""
    per = (hits_cap + SUP_THREADS - 1) // SUP_THREADS
    want = (2048 + n_frames - 1) // n_frames
    return max(1, min(per, want))


def hit_counts(P, forest, model, frames, K, mg, mask):
    """Hit records per frame (k_support's loop bound), from a separate predictor with the debug taps on."""
    with P.HoughPrediction(forest, model) as hp:
        hp.debug_enable(True)
        hp.predict_batch(frames, P.IntrinsicMatrix(K), mg, None, mask)
        return hp.debug_hit_counts(len(frames))


# ---------------------------------------------------------------------------------------------------- (a) every instance
def emit_eb(T):
    return 4 if T <= 4 else 8 if T <= 8 else 10 if T <= 10 else 12 if T <= 12 else 16


# (trees, LS, tree depth): full trees of 2^depth leaves each; LS = 2 needs more than 65 535 leaves in all
FORESTS = [(3, 1, 8), (6, 1, 8), (10, 1, 8), (12, 1, 8), (16, 1, 8), (40, 1, 8), (64, 1, 8), (70, 1, 8),
           (3, 2, 15), (6, 2, 14), (10, 2, 13), (12, 2, 13), (16, 2, 13)]
IW, IH = 128, 112
_forests = {}


def instance_forest(T, ls, depth):
    if (T, ls) not in _forests:
        f = synth.synth_forest(T, depth, synth.FOREST_SEED_BASE + 300 + T, full_depth=depth)
        _forests[(T, ls)] = (f, sr.LeafTables(f))
    return _forests[(T, ls)]


@pytest.mark.parametrize("cam", [False, True], ids=["CAM0", "CAM1"])
@pytest.mark.parametrize("T,ls,depth", FORESTS, ids=[f"EB{emit_eb(T)}-LS{ls}-T{T}" for T, ls, _ in FORESTS])
def test_every_sup_instance(mods, oracle, T, ls, depth, cam):
    _lib, P, TR = mods
    forest, tables = instance_forest(T, ls, depth)
    # the properties that select the instance (dh_launch_emit; dh_api.hip: leaf_ls)
    assert forest.n_trees == T and forest.n_leaves == T << depth
    assert (forest.n_leaves > 65535) == (ls == 2)
    assert {4: T <= 4, 8: 4 < T <= 8, 10: 8 < T <= 10, 12: 10 < T <= 12, 16: T > 12}[emit_eb(T)]
    model = synth.ModelParams(stepwidth=4)
    Ks = cameras_k(IW, IH) if cam else synth.default_intrinsic(IW, IH)
    assert not cam or not all(ef.is_pinhole(K) for K in Ks) and any(ef.is_pinhole(K) for K in Ks)
    frames = frames_for(5, IW, IH, first=40 + T)
    mg, mask = sr.head_guesses(oracle, forest, model, frames, Ks)
    radius = 20
    want, mids = expect(oracle, tables, model, frames, Ks, radius, mg, None, mask)
    assert want["total_mass"].max() > 0 and want["mass"].max() > 0, want
    with P.HoughPrediction(forest, model) as hp:
        if cam:
            with TR.Cameras(Ks) as cams:
                plain = hp.predict_batch_cameras(frames, cams, mg, None, mask)
                poses, sup = hp.predict_batch_cameras_support(frames, cams, radius, mg, None, mask)
        else:
            plain = hp.predict_batch(frames, P.IntrinsicMatrix(Ks), mg, None, mask)
            poses, sup = hp.predict_batch_support(frames, P.IntrinsicMatrix(Ks), radius, mg, None, mask)
    assert poses.tobytes() == plain.tobytes()
    assert np.array_equal(poses["mid_point"], mids)
    assert_support(sup, want, f"k_emit<{emit_eb(T)}, {ls}, {cam}, true>, {T} trees")


def test_instances_meet_partial_support(mods, oracle):
    """The head guesses put some frames of the instance forests' batches between no support and full support."""
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(IW, IH)
    n_partial = 0
    for T, ls, depth in FORESTS:
        forest, tables = instance_forest(T, ls, depth)
        frames = frames_for(5, IW, IH, first=40 + T)
        mg, mask = sr.head_guesses(oracle, forest, model, frames, K)
        want, _ = expect(oracle, tables, model, frames, K, 20, mg, None, mask)
        n_partial += sr.partial(want)
    assert n_partial >= len(FORESTS), n_partial


# ---------------------------------------------------------------------------------------------------- (b) the families
_fam_gpu = {}


def family_gpu_records(P, TR, name, general, decoy):
    """The kernels' SUPPORT_DTYPE [len(radii), n] of a family (once per session), after checking every call's poses."""
    key = (name, general, decoy)
    if key in _fam_gpu:
        return _fam_gpu[key]
    fs = family_support(name, decoy)
    fam = fs["fam"]
    frames = fs["frames"]
    recs = np.zeros_like(fs["recs"])
    with general_path(general):
        with P.HoughPrediction(fam.forest, fam.model, device=0) as hp, \
                (TR.Cameras(fs["Ks"]) if decoy else contextlib.nullcontext()) as cams:
            if decoy:
                plain = hp.predict_batch_cameras(frames, cams, fam.midp, fam.rot)
            else:
                plain = hp.predict_batch(frames, P.IntrinsicMatrix(fam.K), fam.midp, fam.rot)
            if general:
                assert hp.debug_geometry()["uniform"] == 0
            for j, r in enumerate(fs["radii"]):
                if decoy:
                    poses, recs[j] = hp.predict_batch_cameras_support(frames, cams, r, fam.midp, fam.rot)
                else:
                    poses, recs[j] = hp.predict_batch_support(frames, P.IntrinsicMatrix(fam.K), r, fam.midp, fam.rot)
                assert poses.tobytes() == plain.tobytes(), (name, general, decoy, r)
    assert np.array_equal(plain["mid_point"], fs["mids"]), (name, general, decoy)
    _fam_gpu[key] = recs
    return recs


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("name", list(ef.FAMILIES))
def test_families_through_support(mods, name, general):
    _lib, P, TR = mods
    if name in REFUSED:
        fam = family_support(name, False)["fam"]
        with pytest.raises(_lib.DepthheadError, match=REFUSED[name]):      # the refusal of test_gpu_edge_families stands
            P.HoughPrediction(fam.forest, fam.model, device=0)
        return
    for decoy in (False, True):
        fs = family_support(name, decoy)
        got = family_gpu_records(P, TR, name, general, decoy)
        for j, r in enumerate(fs["radii"]):
            assert_support(got[j], fs["recs"][j], (name, "general" if general else "uniform", "decoy" if decoy else "own K", r))


def test_families_reach_on_the_kernels_records(mods):
    """Reach of the whole parametrization above, on the kernels' records (computed here for cases not yet run)."""
    _lib, P, TR = mods
    reach = Reach()
    for name in ef.FAMILIES:
        if name in REFUSED:
            continue
        for general in (False, True):
            for decoy in (False, True):
                reach.add(name, family_support(name, decoy), family_gpu_records(P, TR, name, general, decoy))
    reach.check()


# ---------------------------------------------------------------------------------------------------- (c) launch shapes
def test_one_frame_of_640x480_races_hundreds_of_workgroups(mods, oracle, pose_forest, pose_tables):
    _lib, P, _ = mods
    w, h = 640, 480
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(w, h)
    frames = synth.biwi_batch(1, w, h, first=44)
    mg, mask = sr.head_guesses(oracle, pose_forest, model, frames, K)
    want, mids = expect(oracle, pose_tables, model, frames, K, 30, mg, None, mask)
    assert 0 < want[0]["mass"] < want[0]["total_mass"], want
    nx, ny = model.patch_grid(w, h)
    gx = support_grid_x(1, nx * ny * pose_forest.n_trees)
    hits = hit_counts(P, pose_forest, model, frames, K, mg, mask)
    assert gx >= 256 and hits[0] > 8 * SUP_THREADS, (gx, hits)         # hundreds of workgroups, some of them with records
    with P.HoughPrediction(pose_forest, model) as hp:
        plain = hp.predict_batch(frames, P.IntrinsicMatrix(K), mg, None, mask)
        poses, sup = hp.predict_batch_support(frames, P.IntrinsicMatrix(K), 30, mg, None, mask)
    assert poses.tobytes() == plain.tobytes() and np.array_equal(poses["mid_point"], mids)
    assert_support(sup, want, "640 x 480")


def test_grid_stride_loop_runs_several_passes(mods, oracle, torch_dev, pose_forest, pose_tables):
    """512 frames of 320 x 240 at stride 2 in one launch (no forking): 4 workgroups per frame, so a frame with more than
    1024 hit records takes each workgroup through the loop more than once."""
    torch, dev = torch_dev
    _lib, P, _ = mods
    w, h, n = 320, 240, 512
    model = synth.ModelParams(stepwidth=2)
    K = synth.default_intrinsic(w, h)
    base = frames_for(8, w, h, first=40)
    idx = np.random.RandomState(11).randint(0, 8, n)              # not periodic: a misplaced record shows
    bg, bm = sr.head_guesses(oracle, pose_forest, model, base, K)
    want8, _ = expect(oracle, pose_tables, model, base, K, 20, bg, None, bm)
    assert sr.partial(want8) >= 3, want8
    nx, ny = model.patch_grid(w, h)
    gx = support_grid_x(n, nx * ny * pose_forest.n_trees)
    hits = hit_counts(P, pose_forest, model, base, K, bg, bm)
    assert gx == 4 and hits.max() > 2 * gx * SUP_THREADS, (gx, hits)    # some frame: 3 passes or more
    assert (hits[np.unique(idx)] > gx * SUP_THREADS).sum() >= 4, hits
    ft = torch.from_numpy(base[idx]).to(dev)
    gm, gk = torch.from_numpy(bg[idx].copy()).to(dev), torch.from_numpy(bm[idx].copy()).to(dev)
    out = torch.zeros(n * SB, dtype=torch.uint8, device=dev)
    plain = torch.zeros_like(out)
    sup = torch.zeros(n * SB, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    with P.HoughPrediction(pose_forest, model) as hp:
        hp.set_forking(1)
        hp.predict_batch_device(ft.data_ptr(), n, w, h, P.IntrinsicMatrix(K), plain.data_ptr(), gm.data_ptr(), None, gk.data_ptr(), stream=s)
        hp.predict_batch_support_device(ft.data_ptr(), n, w, h, P.IntrinsicMatrix(K), out.data_ptr(), sup.data_ptr(), 20,
                                        gm.data_ptr(), None, gk.data_ptr(), stream=s)
        torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    assert_support(sup.cpu().numpy().view(_lib.SUPPORT_DTYPE), want8[idx], "512 frames, 4 workgroups per frame")


_CHILD_2048 = r"""
import sys
import numpy as np
import torch
from depthhead_amd import synth
from depthhead_amd.prediction import HoughPrediction, IntrinsicMatrix
d = np.load(sys.argv[1])
frames, mg, mask, K = d["base"][d["idx"]], d["mg"], d["mask"], d["K"]
n, h, w = frames.shape
dev = torch.device("cuda", 0)
ft = torch.from_numpy(frames).to(dev)
gm, gk = torch.from_numpy(mg).to(dev), torch.from_numpy(mask).to(dev)
out = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
plain = torch.zeros_like(out)
sup = torch.zeros_like(out)
forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)
with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp:
    hp.set_forking(1)
    s = torch.cuda.current_stream().cuda_stream
    hp.predict_batch_device(ft.data_ptr(), n, w, h, IntrinsicMatrix(K), plain.data_ptr(), gm.data_ptr(), None, gk.data_ptr(), stream=s)
    hp.predict_batch_support_device(ft.data_ptr(), n, w, h, IntrinsicMatrix(K), out.data_ptr(), sup.data_ptr(), 20, gm.data_ptr(),
                                    None, gk.data_ptr(), stream=s)
    torch.cuda.synchronize()
np.savez(sys.argv[2], out=out.cpu().numpy(), plain=plain.cpu().numpy(), sup=sup.cpu().numpy())
print("child ok")
"""


def test_one_workgroup_per_frame(mods, oracle, pose_forest, pose_tables, tmp_path):
    """2048 frames of 320 x 240 in one launch (DH_MAX_RESIDENT_FRAMES = 2048, no forking, a fresh child process): one
    workgroup per frame walks all of its frame's records, in several runs of 256."""
    _lib, P, _ = mods
    w, h, n = 320, 240, 2048
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(w, h)
    base = frames_for(8, w, h, first=40)
    idx = np.random.RandomState(13).randint(0, 8, n)
    bg, bm = sr.head_guesses(oracle, pose_forest, model, base, K)
    want8, _ = expect(oracle, pose_tables, model, base, K, 20, bg, None, bm)
    assert sr.partial(want8) >= 3, want8
    nx, ny = model.patch_grid(w, h)
    assert support_grid_x(n, nx * ny * pose_forest.n_trees) == 1
    hits = hit_counts(P, pose_forest, model, base, K, bg, bm)
    assert (hits > 2 * SUP_THREADS).sum() >= 4, hits                  # 3 passes or more of the one workgroup
    np.savez(str(tmp_path / "in.npz"), base=base, idx=idx, mg=bg[idx], mask=bm[idx], K=K)
    script = tmp_path / "child.py"
    script.write_text(_CHILD_2048)
    env = dict(os.environ, DH_MAX_RESIDENT_FRAMES="2048", PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, str(script), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True,
                         text=True, env=env, cwd=ROOT, timeout=600)
    assert res.returncode == 0 and "child ok" in res.stdout, (res.returncode, res.stderr[-3000:])
    got = np.load(tmp_path / "out.npz")
    assert got["out"].tobytes() == got["plain"].tobytes()
    assert_support(got["sup"].view(_lib.SUPPORT_DTYPE), want8[idx], "2048 frames, one workgroup per frame")


# ---------------------------------------------------------------------------------------------------- (d) lifecycle
def test_scratch_lifecycle_on_one_predictor(mods, oracle, torch_dev, pose_forest, pose_tables):
    """One predictor through a sequence of support, plain, rejected, reallocating and forked calls: every support record
    equals a fresh predictor's and the restatement's, so the scratch is back to zero after each call."""
    import ctypes as C
    torch, dev = torch_dev
    _lib, P, _ = mods
    model = synth.ModelParams(stepwidth=4)

    def case(n, w, h, first, radius):
        K = synth.default_intrinsic(w, h)
        frames = frames_for(n, w, h, first=first)
        mg, mask = sr.head_guesses(oracle, pose_forest, model, frames, K)
        want, _ = expect(oracle, pose_tables, model, frames, K, radius, mg, None, mask)
        return frames, K, mg, mask, radius, want

    def fresh(c):
        frames, K, mg, mask, radius, _ = c
        with P.HoughPrediction(pose_forest, model) as hq:
            return hq.predict_batch_support(frames, P.IntrinsicMatrix(K), radius, mg, None, mask)

    def check(hp, c, what):
        frames, K, mg, mask, radius, want = c
        poses, sup = hp.predict_batch_support(frames, P.IntrinsicMatrix(K), radius, mg, None, mask)
        fp, fsup = fresh(c)
        assert poses.tobytes() == fp.tobytes(), what
        assert_support(sup, want, what)
        assert sup.tobytes() == fsup.tobytes(), what
        return poses

    big = case(7, 160, 120, 44, 1 << 30)
    small = case(3, 160, 120, 90, 0)
    other = case(4, 128, 112, 60, 20)
    assert big[5]["mass"].max() > 0 and other[5]["mass"].max() > 0 and small[5]["total_mass"].max() > 0
    with P.HoughPrediction(pose_forest, model) as hp:
        check(hp, big, "1: large radius")
        plain = hp.predict_batch(big[0], P.IntrinsicMatrix(big[1]), big[2], None, big[3])
        assert plain.tobytes() == fresh(big)[0].tobytes(), "2: plain call"
        check(hp, small, "3: radius 0, 3 frames")
        with pytest.raises(_lib.DepthheadError, match="radius"):
            hp.predict_batch_support(small[0], P.IntrinsicMatrix(small[1]), -1, small[2], None, small[3])
        lib = _lib.load()
        fr = np.ascontiguousarray(small[0])
        out = np.zeros(3, dtype=_lib.POSE_DTYPE)
        kk = (C.c_float * 9)(*small[1].reshape(9).astype(np.float32))
        assert lib.dh_predict_batch_support(hp._ph, _lib.vp(fr), 3, 160, 120, kk, None, None, None, C.c_uint32(10), _lib.vp(out), None) == -1
        assert b"NULL support" in lib.dh_last_error()
        check(hp, small, "4: after the rejected calls")
        check(hp, other, "5: after a geometry change")
        # 6: forked device call, 48 frames in 3 sub-batches of 16
        n, w, h = 48, 160, 120
        idx = np.random.RandomState(17).randint(0, 7, n)
        frames, K, mg, mask, radius, want = big
        ft = torch.from_numpy(frames[idx]).to(dev)
        gm, gk = torch.from_numpy(mg[idx].copy()).to(dev), torch.from_numpy(mask[idx].copy()).to(dev)
        out_d = torch.zeros(n * SB, dtype=torch.uint8, device=dev)
        sup_d = torch.zeros(n * SB, dtype=torch.uint8, device=dev)
        hp.set_forking(3)
        hp.predict_batch_support_device(ft.data_ptr(), n, w, h, P.IntrinsicMatrix(K), out_d.data_ptr(), sup_d.data_ptr(), radius,
                                        gm.data_ptr(), None, gk.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert_support(sup_d.cpu().numpy().view(_lib.SUPPORT_DTYPE), want[idx], "6: forked")
        hp.set_forking(0)
        check(hp, big, "7: unforked again")


def test_first_support_call_keeps_a_captured_graph(mods, oracle, torch_dev, pose_forest, pose_tables):
    """A plain batch captured into a graph; the predictor's first support call (which allocates the support scratch) with the
    same geometry and fewer frames; the graph still replays, with the same poses."""
    torch, dev = torch_dev
    _lib, P, _ = mods
    w, h, n = 160, 120, 8
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(w, h)
    frames = frames_for(n, w, h, first=40)
    mg, mask = sr.head_guesses(oracle, pose_forest, model, frames, K)
    want, mids = expect(oracle, pose_tables, model, frames, K, 20, mg, None, mask)
    ft = torch.from_numpy(frames).to(dev)
    gm, gk = torch.from_numpy(mg).to(dev), torch.from_numpy(mask).to(dev)
    out = torch.zeros(n * SB, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)
    with P.HoughPrediction(pose_forest, model) as hp:
        hp.reserve(n, w, h)
        hp.graph_capture(ft.data_ptr(), n, w, h, P.IntrinsicMatrix(K), out.data_ptr(), gm.data_ptr(), None, gk.data_ptr())
        hp.graph_launch(st.cuda_stream)
        st.synchronize()
        captured = out.cpu().numpy().copy()
        assert np.array_equal(captured.view(_lib.POSE_DTYPE)["mid_point"], mids)
        m = 5
        poses, sup = hp.predict_batch_support(frames[:m], P.IntrinsicMatrix(K), 20, mg[:m], None, mask[:m])
        assert poses.tobytes() == captured[: m * SB].tobytes()
        assert_support(sup, want[:m], "first support call after the capture")
        out.zero_()
        torch.cuda.synchronize()
        hp.graph_launch(st.cuda_stream)            # accepted: the workspace the graph points into was kept
        st.synchronize()
        assert out.cpu().numpy().tobytes() == captured.tobytes()


# ---------------------------------------------------------------------------------------------------- (e) guard bands
_memo = {}


def expect_memo(oracle, tables, model, frames, Ks, radius, mg, mask, keys):
    """`expect` frame by frame, memoised on keys[i] (the frame's source, camera and guess)."""
    from depthhead_amd._lib import SUPPORT_DTYPE
    recs = np.zeros(len(frames), dtype=SUPPORT_DTYPE)
    for i in range(len(frames)):
        k = (keys[i], radius, mg[i].tobytes(), int(mask[i]))
        if k not in _memo:
            K = Ks[i] if np.ndim(Ks) == 3 else Ks
            _memo[k] = expect(oracle, tables, model, frames[i:i + 1], K, radius, mg[i:i + 1], None, mask[i:i + 1])[0][0]
        recs[i] = _memo[k]
    return recs


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("call", ["batch", "cameras", "tracker"])
def test_support_device_calls_inside_guard_bands(mods, oracle, torch_dev, pose_forest, pose_tables, call, chunks):
    """Frames and guesses between harmful bands (and zero bands), poses and support records at 8 mod 16 and 24 mod 32 between
    guard bands, on a non-default stream: exactly 48 records each, bands intact, records equal to the restatement and the
    same under both kinds of input band."""
    torch, dev = torch_dev
    _lib, P, TR = mods
    w, h, n = 160, 120, 48
    model = synth.ModelParams(stepwidth=4)
    base = frames_for(8, w, h, first=40)
    idx = np.random.RandomState(19 + chunks).randint(0, 8, n)
    frames = base[idx]
    cam_of = np.arange(n) % 5
    Ks = cameras_k(w, h)[cam_of] if call != "batch" else synth.default_intrinsic(w, h)
    keys = [(int(i), int(c) if call != "batch" else -1) for i, c in zip(idx, cam_of)]
    st = torch.cuda.Stream(device=dev)
    runs = []
    for harmful in (True, False):
        out = OutBuf(torch_dev, n * SB, 8, 90)
        sup = OutBuf(torch_dev, n * SB, 24, 91)
        fin = InBuf(torch_dev, frames.nbytes, 2, 17, _harm_u16 if harmful else None)
        gmb = InBuf(torch_dev, n * 12, 4, 23, _harm_f32 if harmful else None)
        gkb = InBuf(torch_dev, n, 1, 29, _harm_u8 if harmful else None)
        got = []
        with P.HoughPrediction(pose_forest, model) as hp, \
                (TR.Cameras(Ks) if call != "batch" else contextlib.nullcontext()) as cams:
            hp.set_forking(chunks)
            if call == "tracker":
                tr = TR.HeadTracker(hp, cams, w, h, prev_guess=True)
                steps = 2
            else:
                steps = 1
                mg, mask = sr.head_guesses(oracle, pose_forest, model, base, synth.default_intrinsic(w, h))
                mg, mask = mg[idx].copy(), mask[idx].copy()
                mask[::7] = 0                                     # some frames without a guess
            for t in range(steps):
                out.reset(); sup.reset()
                fin.upload(frames, st)
                if call == "tracker":
                    s0 = tr.state()
                    mg, mask = s0["midp"], s0["mask"]
                    tr.step_support_device(fin.ptr, out.ptr, sup.ptr, 0, radius=20, stream=st.cuda_stream)
                else:
                    gmb.upload(mg, st)
                    gkb.upload(mask, st)
                    if call == "batch":
                        hp.predict_batch_support_device(fin.ptr, n, w, h, P.IntrinsicMatrix(Ks), out.ptr, sup.ptr, 20, gmb.ptr, None,
                                                        gkb.ptr, stream=st.cuda_stream)
                    else:
                        hp.predict_batch_cameras_support_device(fin.ptr, n, w, h, cams, out.ptr, sup.ptr, 20, gmb.ptr, None,
                                                                gkb.ptr, stream=st.cuda_stream)
                st.synchronize()
                fin.released(); gmb.released(); gkb.released()
                tag = (call, chunks, "harmful" if harmful else "zero", t)
                po = out.result(f"poses {tag}").view(_lib.POSE_DTYPE)
                so = sup.result(f"support {tag}").view(_lib.SUPPORT_DTYPE)
                want = expect_memo(oracle, pose_tables, model, frames, Ks, 20, mg, mask, keys)
                assert_support(so, want, tag)
                got.append((po.tobytes(), so.tobytes()))
                if t == 0 and call != "tracker":
                    assert sr.partial(want) >= 4, want
            if call == "tracker":
                tr.close()
        runs.append(got)
    assert runs[0] == runs[1]
