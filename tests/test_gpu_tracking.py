"""Camera batches (dh_predict_batch_cameras) and live tracking (dh_tracker_*) on the GPU, bit-exact against the oracle.

* a table of n copies of one K predicts byte for byte what predict_batch(K) does -- poses and the taps -- on the uniform
  path and with DH_FORCE_GENERAL=1;
* a mixed batch (pinhole cameras of different f and c, one dense non-pinhole K) equals oracle.predict(frame_i, K_i), with
  guesses, across resident slices and across forked sub-batches;
* a tracker's poses and final state equal a sequential restatement of examples/live_prediction.rs:79-101 that calls the
  oracle per (camera, step) with that camera's K, for all four flag combinations; graph replays advance it as direct steps do.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from depthhead_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 120
f32 = np.float32


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import prediction, tracking
    return prediction, tracking


@pytest.fixture(scope="module")
def scene():
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)   # coherent votes (smoke())
    model = synth.ModelParams(stepwidth=4)
    return forest, model


def cameras_k(w=W, h=H):
    """Six pinhole variants and one dense non-pinhole matrix (the general k_vote instance)."""
    K0 = synth.default_intrinsic(w, h).astype(np.float32)
    ks = [K0]
    for fs, cx, cy in [(1.1, 3.0, -2.0), (0.9, -5.0, 4.0), (1.25, 0.5, 0.25), (0.8, 7.0, 1.0), (1.05, -1.5, -3.5)]:
        K = K0.copy()
        K[0, 0] *= fs; K[1, 1] *= fs * 1.02; K[0, 2] += cx; K[1, 2] += cy
        ks.append(K)
    D = K0.copy()
    D[0, 1] = 0.75; D[1, 0] = -0.5; D[2, 0] = 1e-4; D[2, 1] = -2e-4; D[2, 2] = 1.001
    ks.append(D)
    return np.stack(ks)


def frames_for(n, seed):
    return synth.biwi_batch(n, W, H, first=seed)


def guesses(n, seed):
    rs = np.random.RandomState(seed)
    mg = np.stack([rs.uniform(-80, 80, n), rs.uniform(-60, 60, n), rs.uniform(700, 1100, n)], 1).astype(np.float32)
    rg = rs.uniform(-0.5, 0.5, (n, 3))
    mask = rs.randint(0, 4, n).astype(np.uint8)
    return mg, rg, mask


def oracle_pose(oracle, forest, model, frame, K, mg=None, rg=None):
    r = oracle.predict(forest, model, frame, K, mg, rg, taps=False)
    return r.mid_point, r.rotation


def assert_pose(got, mid, rot, what):
    assert np.array_equal(got["mid_point"], mid) and np.array_equal(got["rotation"], rot), (what, got, mid, rot)


@pytest.mark.parametrize("general", [False, True])
def test_copies_of_one_k_equal_predict_batch(mods, scene, general):
    P, T = mods
    forest, model = scene
    n = 5
    frames = frames_for(n, 40)
    K = synth.default_intrinsic(W, H)
    mg, rg, mask = guesses(n, 3)
    if general:
        os.environ["DH_FORCE_GENERAL"] = "1"
    try:
        hp = P.HoughPrediction(forest, model, device=0)
    finally:
        os.environ.pop("DH_FORCE_GENERAL", None)
    with hp, T.Cameras(np.repeat(K[None], n + 2, 0)) as cams:
        out = []
        hp.debug_enable(True)
        for call in (lambda: hp.predict_batch(frames, P.IntrinsicMatrix(K), mg, rg, mask),
                     lambda: hp.predict_batch_cameras(frames, cams, mg, rg, mask)):
            poses = call()
            out.append(dict(poses=poses.tobytes(), leaf=hp.debug_leaf_indices(n, W, H), grids=hp.debug_grids(n),
                            guesses=hp.debug_guesses(n), flags=hp.debug_patch_flags(n, W, H)))
        if general:
            assert hp.debug_geometry()["uniform"] == 0
    a, b = out
    assert a["poses"] == b["poses"]
    assert np.array_equal(a["leaf"], b["leaf"]) and np.array_equal(a["flags"], b["flags"])
    assert np.array_equal(a["grids"][0], b["grids"][0]) and np.array_equal(a["grids"][1], b["grids"][1])
    assert np.array_equal(a["guesses"], b["guesses"])


def test_mixed_cameras_match_the_oracle(mods, scene, oracle):
    P, T = mods
    forest, model = scene
    Ks = cameras_k()
    n = len(Ks)
    frames = frames_for(n, 60)
    mg, rg, mask = guesses(n, 5)
    with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(Ks) as cams:
        poses = hp.predict_batch_cameras(frames, cams, mg, rg, mask)
        plain = hp.predict_batch_cameras(frames, cams)
    for i in range(n):
        m = mg[i] if mask[i] & 1 else None
        r = rg[i] if mask[i] & 2 else None
        assert_pose(poses[i], *oracle_pose(oracle, forest, model, frames[i], Ks[i], m, r), f"frame {i} with guesses")
        assert_pose(plain[i], *oracle_pose(oracle, forest, model, frames[i], Ks[i]), f"frame {i}")


def test_mixed_cameras_device_batch_forked(mods, scene, oracle):
    """>= 512 frames in two forked sub-batches: every frame equals the single-K batch of its own camera (itself checked against
    the oracle on a sample here)."""
    import torch
    P, T = mods
    forest, model = scene
    Ks = cameras_k()
    n = 520
    base = frames_for(13, 80)
    frames = base[np.arange(n) % 13]
    cam_of = (np.arange(n) * 5) % len(Ks)
    mg, rg, mask = guesses(n, 9)
    with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(Ks[cam_of]) as cams:
        hp.set_forking(2)
        dev = torch.device("cuda:0")
        fr = torch.from_numpy(frames).to(dev)
        g = [torch.from_numpy(x).to(dev) for x in (mg, rg, mask)]
        out = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
        hp.predict_batch_cameras_device(fr.data_ptr(), n, W, H, cams, out.data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
                                        g[2].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=P.POSE_DTYPE)
        hp.set_forking(1)
        for c in range(len(Ks)):
            idx = np.flatnonzero(cam_of == c)
            ref = hp.predict_batch(frames[idx], P.IntrinsicMatrix(Ks[c]), mg[idx], rg[idx], mask[idx])
            assert got[idx].tobytes() == ref.tobytes(), f"camera {c}"
    for i in list(range(0, n, 97)) + [n - 1]:
        m = mg[i] if mask[i] & 1 else None
        r = rg[i] if mask[i] & 2 else None
        assert_pose(got[i], *oracle_pose(oracle, forest, model, frames[i], Ks[cam_of[i]], m, r), f"frame {i}")


def test_mixed_cameras_across_resident_slices(scene, oracle, tmp_path):
    """DH_MAX_RESIDENT_FRAMES = 3 in a fresh child process: the slices offset the camera as they offset the guesses."""
    forest, model = scene
    Ks = cameras_k()
    n = len(Ks)
    frames = frames_for(n, 100)
    mg, rg, mask = guesses(n, 11)
    np.savez(str(tmp_path / "in.npz"), frames=frames, Ks=Ks, mg=mg, rg=rg, mask=mask)
    code = (
        "import numpy as np, sys, json\n"
        "from depthhead_amd import synth\n"
        "from depthhead_amd.prediction import HoughPrediction\n"
        "from depthhead_amd.tracking import Cameras\n"
        "d = np.load(sys.argv[1])\n"
        f"forest = synth.fit_forest(6, 10, {synth.FOREST_SEED_BASE + 9}, n_frames=12, subset=1500)\n"
        "with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, Cameras(d['Ks']) as cams:\n"
        "    p = hp.predict_batch_cameras(d['frames'], cams, d['mg'], d['rg'], d['mask'])\n"
        "print(json.dumps({'mid': p['mid_point'].tolist(), 'rot': p['rotation'].tolist()}))\n")
    env = dict(os.environ, DH_MAX_RESIDENT_FRAMES="3")
    res = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz")], capture_output=True, text=True, env=env,
                         cwd=ROOT, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    for i in range(n):
        m = mg[i] if mask[i] & 1 else None
        r = rg[i] if mask[i] & 2 else None
        mid, rot = oracle_pose(oracle, forest, model, frames[i], Ks[i], m, r)
        assert np.array_equal(np.array(got["mid"][i], dtype=np.float32), mid) and np.array_equal(np.array(got["rot"][i]), rot), i


# ---------------------------------------------------------------------------------------------------- tracking
STEPS, RESET_AT, RESET_CAM, EMPTY_CAM, ABSENT_CAM = 12, 6, 3, 2, 4
ABSENT_STEPS = (3, 4, 7)


def track_frames():
    """[STEPS, C, H, W]: camera 0 holds one head and jumps to another mid-sequence; camera 1 sees a new frame every step;
    camera 2 is empty; cameras 3 .. 6 alternate between two frames."""
    Ks = cameras_k()
    C = len(Ks)
    pool = frames_for(8, 200)
    out = np.zeros((STEPS, C, H, W), dtype=np.uint16)
    seq = frames_for(STEPS, 300)
    for t in range(STEPS):
        out[t, 0] = pool[0] if t < STEPS // 2 else pool[1]
        out[t, 1] = seq[t]
        for c in range(3, C):
            out[t, c] = pool[2 + (c % 3)] if t % 2 == 0 else pool[2 + ((c + 1) % 3)]
    return Ks, out


def present_at(t, C):
    p = np.ones(C, dtype=np.uint8)
    if t in ABSENT_STEPS:
        p[ABSENT_CAM] = 0
    return p


def live_loop_restatement(oracle, forest, model, Ks, frames, prev_guess, sluggish):
    """examples/live_prediction.rs:62-101 per camera, with the tracker's reset and absent steps."""
    C = len(Ks)
    midp = [np.zeros(3, np.float32) for _ in range(C)]
    rot = [None] * C
    poses = []
    held = 0
    for t in range(frames.shape[0]):
        if t == RESET_AT:
            midp[RESET_CAM] = np.zeros(3, np.float32); rot[RESET_CAM] = None
        pres = present_at(t, C)
        step = []
        for c in range(C):
            mg = midp[c] if prev_guess and midp[c][2] > f32(500.0) else None          # :79-86
            rg = rot[c] if prev_guess else None                                         # :101 (None before the first frame)
            mid, r = oracle_pose(oracle, forest, model, frames[t, c], Ks[c], mg, rg)
            step.append((mid, r))
            if not pres[c]:
                continue
            d = (abs(f32(mid[0] - midp[c][0])) + abs(f32(mid[1] - midp[c][1]))) + abs(f32(mid[2] - midp[c][2]))
            if not sluggish or f32(d) < f32(100.0) or midp[c][2] < f32(500.0):       # :92-99
                midp[c] = mid.astype(np.float32).copy()
            else:
                held += 1
            rot[c] = r.copy()
        poses.append(step)
    return poses, midp, rot, held


@pytest.mark.parametrize("prev_guess,sluggish", [(False, False), (True, False), (False, True), (True, True)])
def test_tracker_follows_the_live_loop(mods, scene, oracle, prev_guess, sluggish):
    import torch
    P, T = mods
    forest, model = scene
    Ks, frames = track_frames()
    C = len(Ks)
    ref_poses, ref_midp, ref_rot, held = live_loop_restatement(oracle, forest, model, Ks, frames, prev_guess, sluggish)
    device_steps = prev_guess != sluggish        # two combinations through the device entry point, two through the host one
    with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(Ks) as cams, \
            T.HeadTracker(hp, cams, W, H, prev_guess=prev_guess, sluggish=sluggish) as tr:
        dev = torch.device("cuda:0")
        out = torch.zeros(C * 40, dtype=torch.uint8, device=dev)
        for t in range(STEPS):
            if t == RESET_AT:
                tr.reset(RESET_CAM)
            pres = present_at(t, C)
            if device_steps:
                fr = torch.from_numpy(frames[t]).to(dev)
                pr = torch.from_numpy(pres).to(dev)
                tr.step_device(fr.data_ptr(), out.data_ptr(), pr.data_ptr())
                torch.cuda.synchronize()
                poses = np.frombuffer(out.cpu().numpy().tobytes(), dtype=P.POSE_DTYPE)
            else:
                poses = tr.step(frames[t], pres)
            for c in range(C):
                assert_pose(poses[c], *ref_poses[t][c], f"step {t} camera {c}")
        st = tr.state()
    for c in range(C):
        assert np.array_equal(st["midp"][c].view(np.uint32), ref_midp[c].view(np.uint32)), c
        assert bool(st["has_rot"][c]) == (ref_rot[c] is not None), c
        if ref_rot[c] is not None:
            assert np.array_equal(st["rot"][c], ref_rot[c]), c
        want = (1 if prev_guess and ref_midp[c][2] > f32(500) else 0) | (2 if prev_guess and ref_rot[c] is not None else 0)
        assert st["mask"][c] == want, c
    # the scenario reaches what it is built for: an empty camera never offers a midpoint guess, --sluggish holds some steps
    assert ref_midp[EMPTY_CAM][2] < 500
    assert held > 0 or not (sluggish and not prev_guess)


def test_graph_replays_advance_the_tracker_like_direct_steps(mods, scene):
    import torch
    P, T = mods
    forest, model = scene
    Ks, frames = track_frames()
    C = len(Ks)
    dev = torch.device("cuda:0")
    fr = torch.from_numpy(frames[0]).to(dev)
    pres = torch.from_numpy(present_at(3, C)).to(dev)
    N = 5
    with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(Ks) as cams:
        out_d = torch.zeros(C * 40, dtype=torch.uint8, device=dev)
        out_g = torch.zeros(C * 40, dtype=torch.uint8, device=dev)
        with T.HeadTracker(hp, cams, W, H, prev_guess=True, sluggish=True) as direct:
            seq_d = []
            for _ in range(N):
                direct.step_device(fr.data_ptr(), out_d.data_ptr(), pres.data_ptr())
                torch.cuda.synchronize()
                seq_d.append(out_d.cpu().numpy().tobytes())
            st_d = direct.state()
        with T.HeadTracker(hp, cams, W, H, prev_guess=True, sluggish=True) as graph:
            graph.capture(fr.data_ptr(), out_g.data_ptr(), pres.data_ptr())
            seq_g = []
            for _ in range(N):
                hp.graph_launch()
                torch.cuda.synchronize()
                seq_g.append(out_g.cpu().numpy().tobytes())
            st_g = graph.state()
            assert seq_g == seq_d
            for k in ("midp", "rot", "mask", "has_rot"):
                assert np.array_equal(st_g[k], st_d[k]), k
            assert len(set(seq_d)) > 1 or st_d["mask"].any()    # the guesses took effect
            hp.reserve(4 * C, W, H)                             # a larger workspace: the capture is stale
            with pytest.raises(P._lib.DepthheadError) as ei:
                hp.graph_launch()
            assert ei.value.code == -6


def test_camera_call_errors(mods, scene, hip_lib):
    import ctypes as C
    import torch
    P, T = mods
    forest, model = scene
    Ks = cameras_k()
    frames = frames_for(len(Ks) + 1, 10)
    with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(Ks[:3]) as cams:
        with pytest.raises(P._lib.DepthheadError) as ei:
            hp.predict_batch_cameras(frames[:4], cams)                 # more frames than cameras
        assert ei.value.code == -1 and "cameras" in str(ei.value)
        out = np.zeros(3, dtype=P.POSE_DTYPE)
        assert hip_lib.dh_predict_batch_cameras(hp._ph, None, 3, W, H, cams._h, None, None, None, P.vp(out)) == -1
        assert hip_lib.dh_predict_batch_cameras(hp._ph, P.vp(frames), 3, W, H, None, None, None, None, P.vp(out)) == -1
        with T.HeadTracker(hp, cams, W, H) as tr:
            assert hip_lib.dh_tracker_step(hp._ph, tr._h, None, W, H, None, P.vp(out)) == -1
            assert hip_lib.dh_tracker_step(hp._ph, tr._h, P.vp(frames), W, H, None, None) == -1
            assert hip_lib.dh_tracker_reset(tr._h, 3, None) == -1
            with pytest.raises(P._lib.DepthheadError):
                tr.reset(-2)
        if torch.cuda.device_count() < 2:
            return
        with T.Cameras(Ks[:3], device=1) as other:
            with pytest.raises(P._lib.DepthheadError) as ei:
                hp.predict_batch_cameras(frames[:3], other)
            assert ei.value.code == -1 and "device" in str(ei.value)
            h = C.c_void_p()
            assert hip_lib.dh_tracker_create(other._h, C.c_uint32(1), C.byref(h)) == 0
            assert hip_lib.dh_tracker_step(hp._ph, h, P.vp(frames), W, H, None, P.vp(out)) == -1
            hip_lib.dh_tracker_destroy(h)
