"""The fit tracker on the GPU against its restatement (tests/fit_track_ref.py): every field of every
record and every byte of the state after every step -- no tolerance.  Three cameras (one with a matrix that is no pinhole)
over six steps of tests/fit_track_scenes.py's moving head, with a head gone and back, an absent camera and invalid
detections; the whole step behind a synth forest, whose device poses and support are fed to the restatement; 96x96 frames
with models of 1, 257 and 1025 points (the last streamed, not staged in LDS); every start kind in one launch; the host calls
against their _device twins on a side stream; outputs between guard bands through skewed pointers; reset of one camera and of
all; two runs of one sequence; one step captured in a graph; the refusals that need a tracker."""
import ctypes as C
import functools

import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import fit_track_ref as ft
import fit_track_scenes as sc
from gpu_kit import guarded, same_records, to_device, untouched
from depthhead_amd import _lib, fit, prediction, synth, tracking

pytestmark = pytest.mark.gpu

W, H, STEPS = 160, 120, 6
REC, STATE, POSE, SUP = _lib.FIT_TRACK_RECORD_DTYPE, _lib.FIT_TRACK_STATE_DTYPE, _lib.POSE_DTYPE, _lib.SUPPORT_DTYPE


@functools.lru_cache(maxsize=None)
def cameras_K():
    K = synth.default_intrinsic(W, H)
    Ks = np.stack([K, K, K]).astype(np.float32)
    Ks[1, 0, 0] *= 1.3; Ks[1, 1, 1] *= 0.8; Ks[1, 0, 2] += 11.5
    Ks[2, 0, 1] = 3.0; Ks[2, 2, 0] = 1e-4                             # a matrix that is no pinhole
    Ks.setflags(write=False)
    return Ks


@functools.lru_cache(maxsize=None)
def main_sequence():
    """(frames [STEPS, 3, H, W], poses [STEPS, 3], support [STEPS, 3], present [STEPS, 3]).  Camera 0: the plain sequence.
    Camera 1: the head gone for frames 3 and 4, the detection invalid at frame 4.  Camera 2 (no pinhole): absent at steps 2 - 3,
    its detection invalid at step 0."""
    Ks = cameras_K()
    seqs = [sc.sequence(W, H, 8000 + c, steps=STEPS, gone=(3, 4) if c == 1 else (), K_key=tuple(Ks[c].reshape(9).tolist())) for c in range(3)]
    frames = np.stack([s[0] for s in seqs], axis=1)
    poses = np.stack([s[4] for s in seqs], axis=1)
    sup = np.stack([sc.good_support(3) for _ in range(STEPS)])
    sup["mass"][4, 1] = 0
    sup["windows"][0, 2] = 0
    present = np.ones((STEPS, 3), np.uint8)
    present[2:4, 2] = 0
    for a in (frames, poses, sup, present):
        a.setflags(write=False)
    return frames, poses, sup, present


def model_points(kind):
    v2, _, n2 = fs.head(2)
    if kind == "head2":
        return v2, n2
    if kind == "one":
        front = int(np.argmin(v2[:, 2]))
        return v2[front:front + 1].copy(), n2[front:front + 1].copy()
    if kind == "1025":                                                # the first model past the fit's LDS staging budget of 1024
        v4, _, n4 = fs.head(4)
        return v4[:1025].copy(), n4[:1025].copy()
    v3, _, n3 = fs.head(3)
    return v3[:257].copy(), n3[:257].copy()


@pytest.fixture(scope="module")
def gpu():
    angles = fit.angles()
    with tracking.Cameras(cameras_K()) as cams, fit.Model(*model_points("head2")) as model:
        yield cams, model, angles


def reference(angles, Ks=None, kind="head2", flags=0, **prm):
    pts, nrm = model_points(kind)
    return ft.Tracker(cameras_K() if Ks is None else Ks, pts, nrm, angles, flags=flags, prm=ft.params(**prm))


def ref_fit_params(prm):
    return fr.params() if prm is None else fr.params(prm.coarse_iterations, prm.iterations, (prm.gate[0], prm.gate[1]), prm.lam, prm.min_points)


def kinds(rec):
    return (np.asarray(rec["status"]) & 0xFF).tolist()


def run_both(tr, ref, frames, poses, sup, present, fit_params=None, steps=None):
    """Every step on the GPU (host call) and in the restatement; records and the state compared after each.  Returns the records."""
    out = []
    for k in range(len(frames) if steps is None else steps):
        pr = None if present is None else present[k]
        got = tr.step_poses(frames[k], poses[k], sup[k], pr, fit_params)
        want = ref.step(frames[k], poses[k], sup[k], pr, ref_fit_params(fit_params))
        same_records(got, want, f"records of step {k}")
        same_records(tr.state(), ref.state, f"state after step {k}")
        out.append(got)
    return np.stack(out)


def test_main_sequence_three_cameras(gpu):
    cams, model, angles = gpu
    frames, poses, sup, present = main_sequence()
    with fit.FitTracker(cams, model, W, H) as tr:
        assert not np.frombuffer(tr.state().tobytes(), np.uint8).any()
        rec = run_both(tr, reference(angles), frames, poses, sup, present)
    F, C, R, N, A = ft.FITTED, ft.CARRIED, ft.REJECTED, ft.NONE, ft.ABSENT
    print([kinds(r) for r in rec])
    assert [kinds(r)[0] for r in rec] == [F, C, C, C, C, C]
    assert [kinds(r)[1] for r in rec] == [F, C, C, R, N, F]
    assert [kinds(r)[2] for r in rec][:4] == [N, F, A, A] and kinds(rec[4])[2] in (C, R)
    assert rec["status"][3, 1] == R | ft.BAD_STATUS | ft.BAD_POINTS
    assert (rec["instance"]["frame"][rec["status"] & 0xFF == C] == np.nonzero(rec["status"] & 0xFF == C)[1]).all()


def test_motion_flag_and_other_parameters(gpu):
    cams, model, angles = gpu
    frames, poses, sup, present = main_sequence()
    with fit.FitTracker(cams, model, W, H, motion=True) as tr:
        run_both(tr, reference(angles, flags=ft.MOTION), frames, poses, sup, present)
    prm = dict(iterations_tracked=3, keep_points=60, rms_max=2.0, max_jump=91.0, conf=(1, 10), min_windows=10, max_coast=1)
    fp = fit.fit_params(coarse_iterations=3, iterations=5, gate=(100.0, 30.0), lam=0.01, min_points=20)
    with fit.FitTracker(cams, model, W, H, scale=1.02, motion=True, params=fit.fit_track_params(**prm)) as tr:
        ref = reference(angles, flags=ft.MOTION, **prm)
        ref.scale = np.float32(1.02)
        rec = run_both(tr, ref, frames, poses, sup, present, fp)
    assert (rec["status"] & (ft.BAD_RMS | ft.BAD_JUMP | ft.BAD_POINTS)).any()


@functools.lru_cache(maxsize=None)
def forest():
    return synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)


@pytest.mark.parametrize("radius,conf", [(30, (1, 50)), (100, (0, 1))])
def test_whole_step_behind_a_synth_forest(gpu, radius, conf):
    """dh_fit_tracker_step: the forest's poses and support come from the device and are fed to the restatement."""
    cams, model, angles = gpu
    frames, _, _, present = main_sequence()
    seen = []
    with prediction.HoughPrediction(forest(), synth.ModelParams(stepwidth=4)) as hp, \
            fit.FitTracker(cams, model, W, H, params=fit.fit_track_params(conf=conf)) as tr:
        ref = reference(angles, conf=conf)
        for k in range(STEPS):
            poses, sup, got = tr.step(hp, frames[k], present[k], radius=radius)
            plain_p, plain_s = hp.predict_batch_cameras_support(frames[k], cams, radius=radius)
            same_records(poses, plain_p, "poses"); same_records(sup, plain_s, "support")
            want = ref.step(frames[k], poses, sup, present[k])
            same_records(got, want, f"records of step {k}")
            same_records(tr.state(), ref.state, f"state after step {k}")
            seen.append(kinds(got))
    print(radius, conf, seen)
    assert all(s[2] == ft.ABSENT for s in seen[2:4])


@pytest.mark.parametrize("kind,points", [("one", 1), ("257", 257), ("1025", 1025)])
def test_96x96_one_camera(gpu, kind, points):
    _, _, angles = gpu
    frames, K, pos, Rs, poses = sc.sequence(96, 96, 8010, steps=3)
    pts, nrm = model_points(kind)
    assert len(pts) == points
    with tracking.Cameras(K[None]) as cams, fit.Model(pts, nrm) as model, fit.FitTracker(cams, model, 96, 96) as tr:
        ref = reference(angles, Ks=K[None], kind=kind)
        rec = run_both(tr, ref, frames[:, None], poses[:, None], np.stack([sc.good_support()] * 3), None)
    if points == 1:
        want = ft.REJECTED | ft.BAD_STATUS | ft.BAD_POINTS
        assert (rec["status"] & 0xFFFFFBFF == want).all() and (rec["fit"]["points"] <= 1).all()      # (the one point may miss the rms limit too)
    else:
        assert kinds(rec[:, 0]) == [ft.FITTED, ft.CARRIED, ft.CARRIED]


def test_every_start_kind_in_one_launch(gpu):
    cams, model, angles = gpu
    frames, poses, _, _ = main_sequence()
    sup = np.stack([sc.good_support(3) for _ in range(3)])
    sup["total_mass"][0, 1:] = 0                                      # step 0: only camera 0 is detected
    sup["mass"][1, 2] = 19                                            # step 1: camera 2 just below 1 / 50
    sup["mass"][2, 2] = 20                                            # step 2: exactly 1 / 50
    with fit.FitTracker(cams, model, W, H) as tr:
        rec = run_both(tr, reference(angles), frames[:3], poses[:3], sup, None)
    assert [kinds(r) for r in rec] == [[ft.FITTED, ft.NONE, ft.NONE], [ft.CARRIED, ft.FITTED, ft.NONE], [ft.CARRIED, ft.CARRIED, ft.FITTED]]
    assert rec["lost"][:, 2].tolist() == [1, 2, 0] and not np.frombuffer(rec[1, 2]["instance"].tobytes(), np.uint8).any()


def test_carried_start_skips_the_coarse_phase(gpu):
    cams, model, angles = gpu
    frames, poses, sup, _ = main_sequence()
    with fit.FitTracker(cams, model, W, H) as tr:
        first = tr.step_poses(frames[0], poses[0], sc.good_support(3))
        second = tr.step_poses(frames[1], poses[1], sc.good_support(3))
    assert (first["status"] == ft.FITTED).all() and (first["fit"]["steps"] == 20).all()
    assert (second["status"] == ft.CARRIED).all() and (second["fit"]["steps"] <= 6).all() and (second["age"] == 2).all()


def test_host_calls_against_device_twins_between_guard_bands(gpu):
    """The core step and the whole step, host call against _device twin on a side stream; the twin's outputs lie between 4 KB
    guard bands at skewed pointers (8 bytes off for the records, the poses and the support) and nothing outside them changes."""
    import torch
    cams, model, angles = gpu
    frames, poses, sup, present = main_sequence()
    stream = torch.cuda.Stream()
    with prediction.HoughPrediction(forest(), synth.ModelParams(stepwidth=4)) as hp, fit.FitTracker(cams, model, W, H) as th, \
            fit.FitTracker(cams, model, W, H) as td, fit.FitTracker(cams, model, W, H) as wh, fit.FitTracker(cams, model, W, H) as wd:
        for k in range(4):
            want = th.step_poses(frames[k], poses[k], sup[k], present[k])
            w_poses, w_sup, w_rec = wh.step(hp, frames[k], present[k])
            d_frames, d_poses, d_sup, d_pr = to_device(frames[k]), to_device(poses[k]), to_device(sup[k]), to_device(present[k])
            rec, rec_p, rec_o = guarded(3 * REC.itemsize, 8)
            rec2, rec2_p, rec2_o = guarded(3 * REC.itemsize, 24)
            po, po_p, po_o = guarded(3 * POSE.itemsize, 8)
            so, so_p, so_o = guarded(3 * SUP.itemsize, 8)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                td.step_device(d_frames.data_ptr(), d_poses.data_ptr(), d_sup.data_ptr(), rec_p, present_ptr=d_pr.data_ptr(), stream=stream.cuda_stream)
                wd.step_device(d_frames.data_ptr(), po_p, so_p, rec2_p, hp=hp, present_ptr=d_pr.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            for buf, off, dt, ref_bytes, what in ((rec, rec_o, REC, want, "core records"), (rec2, rec2_o, REC, w_rec, "whole-step records"),
                                                  (po, po_o, POSE, w_poses, "poses"), (so, so_o, SUP, w_sup, "support")):
                nb = 3 * dt.itemsize
                assert untouched(buf, off, nb), what
                same_records(buf.cpu().numpy()[off:off + nb].view(dt), ref_bytes, f"{what} of step {k}")
            same_records(td.state(), th.state(), "core state"); same_records(wd.state(), wh.state(), "whole-step state")


def test_reset_and_two_runs_of_one_sequence(gpu):
    cams, model, angles = gpu
    frames, poses, sup, present = main_sequence()
    with fit.FitTracker(cams, model, W, H) as tr:
        ref = reference(angles)
        first = run_both(tr, ref, frames, poses, sup, present)
        state = tr.state()
        tr.reset(1); ref.reset(1)
        same_records(tr.state(), ref.state, "state after the reset of camera 1")
        assert not np.frombuffer(tr.state()[1].tobytes(), np.uint8).any() and tr.state()[0].tobytes() == state[0].tobytes()
        run_both(tr, ref, frames, poses, sup, present, steps=2)
        tr.reset(); ref.reset()
        assert not np.frombuffer(tr.state().tobytes(), np.uint8).any()
        second = run_both(tr, ref, frames, poses, sup, present)
        assert first.tobytes() == second.tobytes() and tr.state().tobytes() == state.tobytes()


def test_one_step_captured_in_a_graph(gpu):
    """The core step's three launches captured with torch.cuda.graph; each replay is one step and equals the eager step."""
    import torch
    cams, model, angles = gpu
    frames, poses, sup, present = main_sequence()
    with fit.FitTracker(cams, model, W, H) as eager, fit.FitTracker(cams, model, W, H) as tr:
        d_frames, d_poses, d_sup = to_device(frames[0]), to_device(poses[0]), to_device(sup[0])
        d_rec = torch.zeros(3 * REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tr.step_device(d_frames.data_ptr(), d_poses.data_ptr(), d_sup.data_ptr(), d_rec.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        tr.reset()                                                     # whatever the capture itself ran or did not run
        torch.cuda.synchronize()
        for k in range(3):
            d_frames.copy_(to_device(frames[k])); d_poses.copy_(to_device(poses[k])); d_sup.copy_(to_device(sup[k]))
            g.replay()
            torch.cuda.synchronize()
            want = eager.step_poses(frames[k], poses[k], sup[k])
            same_records(d_rec.cpu().numpy().view(REC), want, f"replay {k}")
            same_records(tr.state(), eager.state(), f"state after replay {k}")


def test_refusals_that_need_a_tracker(gpu):
    cams, model, angles = gpu
    frames, poses, sup, present = main_sequence()
    lib, vp = _lib.load(), _lib.vp
    with fit.FitTracker(cams, model, W, H) as tr:
        before = tr.step_poses(frames[0], poses[0], sup[0])
        state = tr.state()
        rec = np.full(3 * REC.itemsize, 0xCD, np.uint8)
        f, p, s = np.ascontiguousarray(frames[1]), np.ascontiguousarray(poses[1]), np.ascontiguousarray(sup[1])

        def refused(what, fr_=f, w=W, h=H, po=p, su=s, prm=None, out=rec):
            for name, extra in (("dh_fit_tracker_step_poses", ()), ("dh_fit_tracker_step_poses_device", (None,))):
                rc = getattr(lib, name)(tr._h, vp(fr_), w, h, None, vp(po), vp(su), prm, vp(out), *extra)
                msg = lib.dh_last_error().decode()
                assert rc == -1 and what in msg and name in msg, (name, rc, msg)
            assert (rec == 0xCD).all()

        refused("NULL frames", fr_=None)
        refused("NULL poses or support", po=None)
        refused("NULL poses or support", su=None)
        refused("NULL records", out=None)
        for w, h in ((0, H), (W, 0), (-1, H), (W, _lib.RENDER_MAX_SIZE + 1)):
            refused("frame size", w=w, h=h)
        for kw, what in ((dict(coarse_iterations=33, iterations=32), "above 64"), (dict(gate=(0.0, 25.0)), "gate[0]"),
                         (dict(gate=(120.0, 5000.0)), "gate[1]"), (dict(lam=-1.0), "lambda"), (dict(min_points=5), "min_points 5 below 6")):
            refused(what, prm=C.byref(fit.fit_params(**kw)))
        for cam in (-2, 3):
            with pytest.raises(_lib.DepthheadError) as ei:
                tr.reset(cam)
            assert ei.value.code == -1 and "camera" in str(ei.value)
        assert lib.dh_fit_tracker_state(tr._h, None) == -1 and "NULL" in lib.dh_last_error().decode()
        with prediction.HoughPrediction(forest(), synth.ModelParams(stepwidth=4)) as hp:
            po_, su_ = np.zeros(3, POSE), np.zeros(3, SUP)
            rc = lib.dh_fit_tracker_step(hp._ph, tr._h, vp(f), W, H, None, C.c_uint32(0x80000000), None, vp(po_), vp(su_), vp(rec))
            assert rc == -1 and "radius" in lib.dh_last_error().decode() and (rec == 0xCD).all() and not po_.tobytes().strip(b"\0")
        assert tr.state().tobytes() == state.tobytes()                 # nothing was launched
        assert tr.step_poses(frames[0], poses[0], sup[0], [0, 0, 0])["status"].tolist() == [ft.ABSENT] * 3
    radius = model.info()[1]
    for scale in (float(np.float32(4096.5 / radius)), -float(np.float32(4096.5 / radius))):
        with pytest.raises(_lib.DepthheadError) as ei:
            fit.FitTracker(cams, model, W, H, scale=scale)
        assert ei.value.code == -1 and "mm from its origin" in str(ei.value)
    assert before.dtype == REC
