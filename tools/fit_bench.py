"""Time the fit: `--frames` device-resident frames of `--size`, each a rendered head (`synth.head_mesh(--subdiv)`) and its torso
box, one instance per frame started `--offset` mm and up to `--deg` degrees per axis from the truth, fitted to device outputs.
Prints one JSON line: ms per batch measured with device events around each of `--steps` calls (after `--warmup`), as median,
minimum and maximum over the calls of each of `--runs` repeats, and the mean position / rotation error before and after."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--offset", type=float, default=90.0)
    ap.add_argument("--deg", type=float, default=25.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import _lib, fit, render, synth, training
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    items, truth, start = [], [], []
    for f in range(a.frames):
        pos, rot = training.rendered_pose(w, h, training.RENDER_SEED_BASE + f)
        R = render.euler_to_matrix(rot)
        items.append((f, 0, R, pos, 1.0, True))
        items.append((f, 1, np.eye(3), pos, 1.0, False))
        u = synth.SplitMix(31337 + f).uniform(6)
        d = 2.0 * u[:3] - 1.0
        R0 = render.euler_to_matrix(a.deg * (2.0 * u[3:] - 1.0)).astype(np.float64) @ R.astype(np.float64)
        truth.append((pos.astype(np.float64), R.astype(np.float64)))
        start.append((f, 0, R0, pos + a.offset * d / np.sqrt((d * d).sum()), 1.0, False))
    inst = render.instances(start)

    def errors(x):
        p = np.array([np.linalg.norm(x["t"][i] - truth[i][0]) for i in range(a.frames)])
        c = np.array([(np.trace(truth[i][1].T @ x["R"][i].reshape(3, 3).astype(np.float64)) - 1.0) / 2.0 for i in range(a.frames)])
        return float(p.mean()), float(p.max()), float(np.degrees(np.arccos(np.clip(c, -1, 1))).mean())

    with render.Mesh(verts, tris) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd, fit.Model.from_mesh(verts, tris) as model, fit.Fitter() as ft:
        frames, _ = rd.render([head, torso], render.instances(items), a.frames, w, h, K, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        torch.cuda.synchronize()
        runs = []
        for _ in range(a.runs):
            for _ in range(a.warmup):
                out, rec = ft.fit(frames, [model], inst, K, device_out=True)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out, rec = ft.fit(frames, [model], inst, K, device_out=True)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            runs.append({"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))})
        out = out.cpu().numpy().view(_lib.RENDER_INSTANCE_DTYPE)
        rec = rec.cpu().numpy().view(_lib.FIT_RECORD_DTYPE)
    med = [r["median_ms"] for r in runs]
    print(json.dumps({"frames": a.frames, "size": a.size, "points": len(verts), "fit_ms": float(np.median(med)), "fit_ms_min_run": min(med),
                      "fit_ms_max_run": max(med), "runs": runs, "frames_per_s": a.frames / (float(np.median(med)) * 1e-3),
                      "status_ok": int((rec["status"] == 0).sum()), "points_used_mean": float(rec["points"].mean()),
                      "steps_mean": float(rec["steps"].mean()),
                      "start_pos_mean_max_rot": errors(inst), "fitted_pos_mean_max_rot": errors(out)}))


if __name__ == "__main__":
    main()
