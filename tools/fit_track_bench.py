"""Time the fit tracker: `--cameras` cameras of `--size`, each seeing a rendered head (`synth.head_mesh(--subdiv)`) and its torso
box, device-resident frames and outputs.  Three things, each as the median (and spread) of `--runs` run medians over `--steps`
calls after `--warmup`, in ms per step of all cameras, measured with device events and, because (c) waits on the host, also with
the host's clock between two synchronisations:
  (a) dh_fit_tracker_step_device in steady state: every camera carried;
  (b) dh_fit_tracker_step_device with every camera re-seeded (a reset before each step);
  (c) what the same costs without the tracker: dh_predict_batch_cameras_support_device, the poses copied back,
      fit.instances_from_poses on the host, dh_fit_depth_cameras_device.
The prediction runs the bench forest (`synth.fit_forest`) without guesses, whose poses need not be near the heads; so that the
fit work is the work of a detector 90 mm off whatever that forest answers, the tracker's state is seeded by one core step from
poses faked as the truth plus `--offset` mm, the tracker believes every detection (conf 0 / 1, no minimum of windows) and never
rejects on the jump (max_jump 4096), and (c) fits from the faked poses.  The statuses and mean step counts of the timed steps
are reported: (b)'s forest starts may end early where the forest's pose is far off, and then (b) understates a real detector's
cost; `core_reseeded` is the core step alone from the faked poses, to be added to `predict` for that case.  One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=256)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--offset", type=float, default=90.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import _lib, fit, render, synth, tracking, training
    from depthhead_amd.prediction import HoughPrediction
    n = a.cameras
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    items = []
    poses = np.zeros(n, _lib.POSE_DTYPE)
    support = np.zeros(n, _lib.SUPPORT_DTYPE)
    support["windows"], support["mass"], support["total_mass"] = 10, 100, 1000
    bin_ = 3.14159 / 60.0
    for f in range(n):
        pos, rot = training.rendered_pose(w, h, training.RENDER_SEED_BASE + f)
        items.append((f, 0, render.euler_to_matrix(rot), pos, 1.0, True))
        items.append((f, 1, np.eye(3), pos, 1.0, False))
        d = 2.0 * synth.SplitMix(31337 + f).uniform(3) - 1.0
        poses["mid_point"][f] = np.round(pos + a.offset * d / np.sqrt((d * d).sum()))
        poses["rotation"][f] = np.round(np.radians(rot.astype(np.float64)) / bin_) * bin_
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)
    prm = fit.fit_track_params(conf=(0, 1), min_windows=0, max_jump=4096.0)
    dev = torch.device("cuda", 0)

    def dbuf(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def timed(fn, before=None):
        """Run medians of fn(): (device-event ms, host-clock ms) per call."""
        ev, host = [], []
        for _ in range(a.runs):
            e, hs = [], []
            for i in range(a.warmup + a.steps):
                if before:
                    before()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    e.append(e0.elapsed_time(e1)); hs.append((t1 - t0) * 1e3)
            ev.append(float(np.median(e))); host.append(float(np.median(hs)))
        return {"event_ms": float(np.median(ev)), "event_ms_runs": [min(ev), max(ev)], "host_ms": float(np.median(host)),
                "host_ms_runs": [min(host), max(host)]}

    with render.Mesh(verts, tris) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd, fit.Model.from_mesh(verts, tris) as model, fit.Fitter() as ft, \
            tracking.Cameras(np.tile(K.reshape(1, 9), (n, 1))) as cams, HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, \
            fit.FitTracker(cams, model, w, h, params=prm) as tr:
        frames, _ = rd.render([head, torso], render.instances(items), n, w, h, K, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        s = torch.cuda.current_stream(dev).cuda_stream
        d_fake_p = torch.from_numpy(poses.view(np.uint8).copy()).to(dev)
        d_fake_s = torch.from_numpy(support.view(np.uint8).copy()).to(dev)
        d_p, d_s, d_r = dbuf(n * 40), dbuf(n * 40), dbuf(n * _lib.FIT_TRACK_RECORD_DTYPE.itemsize)
        host_p = np.zeros(n, _lib.POSE_DTYPE)

        def records():
            torch.cuda.synchronize()
            r = d_r.cpu().numpy().view(_lib.FIT_TRACK_RECORD_DTYPE)
            return {"kinds": np.bincount(r["status"] & 0xFF, minlength=5).tolist(), "steps_mean": float(r["fit"]["steps"].mean())}

        def seed():
            tr.reset(stream=s)
            tr.step_device(frames.data_ptr(), d_fake_p.data_ptr(), d_fake_s.data_ptr(), d_r.data_ptr(), stream=s)

        def whole():
            tr.step_device(frames.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_r.data_ptr(), hp=hp, stream=s)

        def core():
            tr.step_device(frames.data_ptr(), d_fake_p.data_ptr(), d_fake_s.data_ptr(), d_r.data_ptr(), stream=s)

        def predict():
            hp.predict_batch_cameras_support_device(frames.data_ptr(), n, w, h, cams, d_p.data_ptr(), d_s.data_ptr(), stream=s)

        def today():
            predict()
            torch.cuda.synchronize()
            host_p[:] = d_p.cpu().numpy().view(_lib.POSE_DTYPE)            # the round trip: the forest's poses on the host ...
            inst = fit.instances_from_poses(poses)                         # ... (the faked ones are fitted: see above)
            ft.fit(frames, [model], inst, cams, device_out=True)

        out = {"cameras": n, "size": a.size, "points": len(verts)}
        seed()
        out["seeded"] = records()
        out["a_carried"] = timed(whole)
        out["a_carried"].update(records())
        out["b_reseeded"] = timed(whole, before=lambda: tr.reset(stream=s))
        out["b_reseeded"].update(records())
        out["core_reseeded"] = timed(core, before=lambda: tr.reset(stream=s))
        out["core_reseeded"].update(records())
        seed()
        out["core_carried"] = timed(core)
        out["core_carried"].update(records())
        out["predict"] = timed(predict)
        out["c_today"] = timed(today)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
