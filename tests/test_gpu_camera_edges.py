"""Camera tables (dh_predict_batch_cameras[_device]) and tracking (dh_tracker_*) at the edges the single-K path is held to.

(a) every 3-D family of tests/edge_families.py through the CAM instances of k_emit / k_vote / k_region / k_cluster: each
    frame once with the family's K and once with a decoy camera (ef.decoy_cameras), all records pinhole (k_vote<PIN, CAM>) and
    once more with a dense camera added (the general CAM instance), on the uniform path and with DH_FORCE_GENERAL=1; every
    tap of every frame equals oracle/pyref.py with that frame's K;
(b) the camera index where the host and device paths offset it: a host batch of staged upload chunks, the same across
    resident slices in a child process, a forked device batch whose sub-batches take different k_vote instances, and frame
    sizes that are not multiples of 20 (k_vote's approximate cell quotient off);
(c) an all-pinhole tracker under both entry points, and host tracker steps across resident slices with the absent camera in
    the middle slice, against the live-loop restatement of tests/test_gpu_tracking.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_families as ef
from depthhead_amd import synth
from oracle import pyref
from test_edge_pyref import KEYS, decoy_results, family_results
from test_gpu_edge_families import REFUSED, general_path
from test_gpu_tracking import (RESET_AT, RESET_CAM, STEPS, ABSENT_CAM, assert_pose, cameras_k, guesses, live_loop_restatement,
                               oracle_pose, present_at, track_frames)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import prediction, tracking
    return prediction, tracking


@pytest.fixture(scope="module")
def scene():
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)
    return forest, synth.ModelParams(stepwidth=4)


def _dense_like(K):
    D = np.asarray(K, dtype=np.float32).copy()
    D[0, 1] = 0.75; D[1, 0] = -0.5; D[2, 0] = 1e-4; D[2, 1] = -2e-4; D[2, 2] = 1.001
    return D


def _camera_taps(P, T, fam, frames, Ks, midp, rot):
    n, h, w = frames.shape
    with P.HoughPrediction(fam.forest, fam.model, device=0) as hp, T.Cameras(Ks) as cams:
        hp.debug_enable(True)
        poses = hp.predict_batch_cameras(frames, cams, midp, rot)
        leaf, flags = hp.debug_leaf_indices(n, w, h), hp.debug_patch_flags(n, w, h)
        pos_grid, rot_grid = hp.debug_grids(n)
        g = hp.debug_guesses(n)
        tr_mid, st_mid = hp.debug_meanshift(n, 0)
        tr_rot, st_rot = hp.debug_meanshift(n, 1)
        votes = [(P.aggregate_votes(hp.debug_votes(i, 0)), P.aggregate_votes(hp.debug_votes(i, 1))) for i in range(n)]
    return [dict(leaf_idx=leaf[i], patch_flags=flags[i], pos_grid=pos_grid[i], rot_grid=rot_grid[i], guess_mid=g[i, :3],
                 guess_rot=g[i, 3:], mid_cells=votes[i][0], rot_cells=votes[i][1], ms_trace_mid=(tr_mid[i], st_mid[i]),
                 ms_trace_rot=(tr_rot[i], st_rot[i]), mid_point=poses["mid_point"][i], rotation=poses["rotation"][i])
            for i in range(n)]


def _assert_taps(what, got, ref, iterations):
    """The rule of test_gpu_edge_families.test_hip_against_pyref."""
    for k in KEYS:
        if k.startswith("ms_trace"):
            tr, st = got[k]
            n = ref[k].shape[0]
            assert st + 1 >= n or st == iterations, (what, k, st, n)
            assert np.array_equal(tr[:n], ref[k]), (what, k, tr[:n], ref[k])
        else:
            assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("name", [n for n in ef.FAMILIES if n not in REFUSED])
def test_families_through_camera_tables(mods, name, general):
    P, T = mods
    fam, res = family_results(name)
    Ds, dres = decoy_results(name)
    n = fam.frames.shape[0]
    frames = np.repeat(fam.frames, 2, axis=0)                              # frame i with K, then with decoy i
    Ks = np.stack([M for i in range(n) for M in (fam.K, Ds[i])]).astype(np.float32)
    refs = [r for i in range(n) for r in (res[i], dres[i])]
    midp = None if fam.midp is None else np.repeat(fam.midp, 2, axis=0)
    rot = None if fam.rot is None else np.repeat(fam.rot, 2, axis=0)
    runs = [("as given", frames, Ks, midp, rot)]
    if ef.is_pinhole(fam.K):
        # run B: one dense camera more (frame 0 again) sends the whole launch to the general CAM instance
        dense = _dense_like(fam.K)
        with np.errstate(all="ignore"):
            refs_b = refs + [pyref.predict(fam.forest, fam.model, fam.frames[0], dense, *fam.guesses(0))]
        runs.append(("with a dense camera", np.concatenate([frames, fam.frames[:1]]), np.concatenate([Ks, dense[None]]),
                     None if midp is None else np.concatenate([midp, midp[:1]]), None if rot is None else np.concatenate([rot, rot[:1]])))
    it = fam.model.meanshift_iterations
    for label, fr, ks, mg, rg in runs:
        with general_path(general):
            got = _camera_taps(P, T, fam, fr, ks, mg, rg)
        want = refs if len(fr) == len(refs) else refs_b
        for i, (g, r) in enumerate(zip(got, want)):
            _assert_taps((name, label, i), g, r, it)


# ---------------------------------------------------------------------------------------------------- the camera index
def _per_camera_reference(hp, P, frames, Ks, cam_of, mg, rg, mask):
    ref = np.zeros(len(frames), dtype=P.POSE_DTYPE)
    for c in range(len(Ks)):
        idx = np.flatnonzero(cam_of == c)
        if idx.size:
            ref[idx] = hp.predict_batch(frames[idx], P.IntrinsicMatrix(Ks[c]), mg[idx], rg[idx], mask[idx])
    return ref


def _oracle_sample(oracle, forest, model, frames, Ks, cam_of, mg, rg, mask, got, idx):
    for i in idx:
        m = mg[i] if mask[i] & 1 else None
        r = rg[i] if mask[i] & 2 else None
        assert_pose(got[i], *oracle_pose(oracle, forest, model, frames[i], Ks[cam_of[i]], m, r), f"frame {i}")


def _staged_inputs():
    Ks = cameras_k()
    n = 105                                     # dh_chunk_plan_(105, 64): upload chunks [0, 53, 79, 95, 105)
    frames = synth.biwi_batch(15, 160, 120, first=400)[np.arange(n) % 15]
    cam_of = (np.arange(n) * 3) % len(Ks)
    mg, rg, mask = guesses(n, 21)
    return Ks, frames, cam_of, mg, rg, mask


def test_staged_host_batch_offsets_the_camera(mods, scene, oracle):
    P, T = mods
    forest, model = scene
    Ks, frames, cam_of, mg, rg, mask = _staged_inputs()
    with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(Ks[cam_of]) as cams:
        got = hp.predict_batch_cameras(frames, cams, mg, rg, mask)
        ref = _per_camera_reference(hp, P, frames, Ks, cam_of, mg, rg, mask)
    assert got.tobytes() == ref.tobytes()
    _oracle_sample(oracle, forest, model, frames, Ks, cam_of, mg, rg, mask, got, [0, 52, 53, 78, 79, 94, 95, 104])


def test_staged_host_batch_across_resident_slices(mods, scene, oracle, tmp_path):
    """DH_MAX_RESIDENT_FRAMES = 45 in a fresh child: slices [0, 45) [45, 90) [90, 105), each of upload chunks [0, 23) [23, 45)."""
    P, T = mods
    forest, model = scene
    Ks, frames, cam_of, mg, rg, mask = _staged_inputs()
    np.savez(str(tmp_path / "in.npz"), frames=frames, Ks=Ks[cam_of], mg=mg, rg=rg, mask=mask)
    code = (
        "import numpy as np, sys\n"
        "from depthhead_amd import synth\n"
        "from depthhead_amd.prediction import HoughPrediction\n"
        "from depthhead_amd.tracking import Cameras\n"
        "d = np.load(sys.argv[1])\n"
        f"forest = synth.fit_forest(6, 10, {synth.FOREST_SEED_BASE + 9}, n_frames=12, subset=1500)\n"
        "with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, Cameras(d['Ks']) as cams:\n"
        "    p = hp.predict_batch_cameras(d['frames'], cams, d['mg'], d['rg'], d['mask'])\n"
        "np.save(sys.argv[2], p)\n"
        "print('child ok')\n")
    env = dict(os.environ, DH_MAX_RESIDENT_FRAMES="45")
    res = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz"), str(tmp_path / "out.npy")], capture_output=True,
                         text=True, env=env, cwd=ROOT, timeout=600)
    assert res.returncode == 0 and "child ok" in res.stdout, (res.returncode, res.stderr[-2000:])
    got = np.load(tmp_path / "out.npy")
    with P.HoughPrediction(forest, model, device=0) as hp:
        ref = _per_camera_reference(hp, P, frames, Ks, cam_of, mg, rg, mask)
    assert got.tobytes() == ref.tobytes()
    _oracle_sample(oracle, forest, model, frames, Ks, cam_of, mg, rg, mask, got, [44, 45, 67, 68, 89, 90, 104])


def test_forked_device_batch_with_a_pinhole_and_a_general_half(mods, scene, oracle):
    """520 frames in two forked sub-batches [0, 260) and [260, 520): the first sees only pinhole cameras (k_vote<PIN, CAM>),
    the second also the dense one (the general CAM instance)."""
    import torch
    P, T = mods
    forest, model = scene
    Ks = cameras_k()
    dense = len(Ks) - 1
    assert not ef.is_pinhole(Ks[dense]) and all(ef.is_pinhole(K) for K in Ks[:dense])
    n = 520
    frames = synth.biwi_batch(13, 160, 120, first=80)[np.arange(n) % 13]
    i = np.arange(n)
    cam_of = np.where(i < n // 2, (i * 5) % dense, (i * 5) % len(Ks))
    assert (cam_of[n // 2:] == dense).any() and not (cam_of[:n // 2] == dense).any()
    mg, rg, mask = guesses(n, 31)
    with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(Ks[cam_of]) as cams:
        hp.set_forking(2)
        dev = torch.device("cuda:0")
        fr = torch.from_numpy(frames).to(dev)
        g = [torch.from_numpy(x).to(dev) for x in (mg, rg, mask)]
        out = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
        hp.predict_batch_cameras_device(fr.data_ptr(), n, 160, 120, cams, out.data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
                                        g[2].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=P.POSE_DTYPE)
        hp.set_forking(1)
        ref = _per_camera_reference(hp, P, frames, Ks, cam_of, mg, rg, mask)
    assert got.tobytes() == ref.tobytes()
    _oracle_sample(oracle, forest, model, frames, Ks, cam_of, mg, rg, mask, got, [0, 259, 260, 261, 519] + list(range(3, n, 101)))


@pytest.mark.parametrize("w,h", [(150, 113), (201, 152)])
def test_camera_batches_off_the_cell_grid(mods, scene, oracle, w, h):
    """Frame sizes that are not multiples of 20 (no approximate cell quotient) and widths of residues 2 and 1 mod 4."""
    P, T = mods
    forest, model = scene
    Ks = cameras_k(w, h)
    n = 2 * len(Ks)
    frames = synth.biwi_batch(n, w, h, first=500)
    cam_of = np.arange(n) % len(Ks)
    mg, rg, mask = guesses(n, 41)
    for table in (Ks[cam_of], Ks[cam_of][:len(Ks) - 1]):       # with the dense camera, and the all-pinhole prefix
        m = len(table)
        with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(table) as cams:
            got = hp.predict_batch_cameras(frames[:m], cams, mg[:m], rg[:m], mask[:m])
        _oracle_sample(oracle, forest, model, frames, Ks, cam_of, mg, rg, mask, got, range(m))


# ---------------------------------------------------------------------------------------------------- tracking
def _check_state(st, ref_midp, ref_rot, prev_guess, C):
    f32 = np.float32
    for c in range(C):
        assert np.array_equal(st["midp"][c].view(np.uint32), ref_midp[c].view(np.uint32)), c
        assert bool(st["has_rot"][c]) == (ref_rot[c] is not None), c
        if ref_rot[c] is not None:
            assert np.array_equal(st["rot"][c], ref_rot[c]), c
        want = (1 if prev_guess and ref_midp[c][2] > f32(500) else 0) | (2 if prev_guess and ref_rot[c] is not None else 0)
        assert st["mask"][c] == want, c


@pytest.mark.parametrize("device_steps", [False, True])
def test_all_pinhole_tracker_follows_the_live_loop(mods, scene, oracle, device_steps):
    """cameras_k()[:6]: every launch of the tracker takes k_vote<PIN, CAM>."""
    import torch
    P, T = mods
    forest, model = scene
    Ks, frames = track_frames()
    Ks, frames = Ks[:6], frames[:, :6].copy()
    C = len(Ks)
    assert all(ef.is_pinhole(K) for K in Ks)
    ref_poses, ref_midp, ref_rot, _ = live_loop_restatement(oracle, forest, model, Ks, frames, True, True)
    W, H = frames.shape[3], frames.shape[2]
    with P.HoughPrediction(forest, model, device=0) as hp, T.Cameras(Ks) as cams, \
            T.HeadTracker(hp, cams, W, H, prev_guess=True, sluggish=True) as tr:
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
        _check_state(tr.state(), ref_midp, ref_rot, True, C)


def test_host_tracker_steps_across_resident_slices(mods, scene, oracle, tmp_path):
    """DH_MAX_RESIDENT_FRAMES = 3 in a fresh child: the seven cameras in slices [0, 3) [3, 6) [6, 7); the absent camera (4)
    sits in the middle slice, so its `present` byte crosses in the staged copy of that slice."""
    forest, model = scene
    Ks, frames = track_frames()
    C = len(Ks)
    assert 3 <= ABSENT_CAM < 6
    np.savez(str(tmp_path / "in.npz"), frames=frames, Ks=Ks, present=np.stack([present_at(t, C) for t in range(STEPS)]))
    code = (
        "import numpy as np, sys\n"
        "from depthhead_amd import synth\n"
        "from depthhead_amd.prediction import HoughPrediction\n"
        "from depthhead_amd.tracking import Cameras, HeadTracker\n"
        "d = np.load(sys.argv[1])\n"
        f"forest = synth.fit_forest(6, 10, {synth.FOREST_SEED_BASE + 9}, n_frames=12, subset=1500)\n"
        "fr = d['frames']\n"
        "poses = []\n"
        "with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, Cameras(d['Ks']) as cams, \\\n"
        "        HeadTracker(hp, cams, fr.shape[3], fr.shape[2], prev_guess=True, sluggish=True) as tr:\n"
        "    for t in range(fr.shape[0]):\n"
        f"        if t == {RESET_AT}:\n"
        f"            tr.reset({RESET_CAM})\n"
        "        poses.append(tr.step(fr[t], d['present'][t]))\n"
        "    st = tr.state()\n"
        "np.savez(sys.argv[2], poses=np.stack(poses), midp=st['midp'], rot=st['rot'], mask=st['mask'], has_rot=st['has_rot'])\n"
        "print('child ok')\n")
    env = dict(os.environ, DH_MAX_RESIDENT_FRAMES="3")
    res = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True,
                         text=True, env=env, cwd=ROOT, timeout=600)
    assert res.returncode == 0 and "child ok" in res.stdout, (res.returncode, res.stderr[-2000:])
    out = np.load(tmp_path / "out.npz")
    ref_poses, ref_midp, ref_rot, _ = live_loop_restatement(oracle, forest, model, Ks, frames, True, True)
    for t in range(STEPS):
        for c in range(C):
            assert_pose(out["poses"][t][c], *ref_poses[t][c], f"step {t} camera {c}")
    _check_state({k: out[k] for k in ("midp", "rot", "mask", "has_rot")}, ref_midp, ref_rot, True, C)
