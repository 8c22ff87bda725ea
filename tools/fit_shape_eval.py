"""Time one shape step against the fit on the same batch in the same process: `--frames` device-resident
frames of `--size`, each the SUBJECT's head (`synth.head_mesh(--subdiv)` stretched by `--stretch`) and its torso box, one
instance per frame started `--offset` mm and up to `--deg` degrees per axis from the truth.  The generic model is fitted
(dh_fit_depth_device) and one shape step with the first `--fields` fields of `synth.head_basis` is taken over the fitted
instances, all in one subject (dh_fit_shape_device).  Prints one JSON line: ms per call measured with device events around each
of `--steps` calls (after `--warmup`), as the median over the calls of each of `--runs` repeats and the spread of those medians,
for both, their ratio, and the step's record.  `--adapt N` also runs fit.adapt on the first N frames and reports the
coefficients against the stretch."""
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
    ap.add_argument("--fields", type=int, default=4)
    ap.add_argument("--stretch", default="1.08,0.93,1.06")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--offset", type=float, default=15.0)
    ap.add_argument("--deg", type=float, default=6.0)
    ap.add_argument("--adapt", type=int, default=0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import _lib, fit, render, synth, training
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    fields = synth.head_basis(verts)[:a.fields]
    c_true = np.array([float(v) - 1.0 for v in a.stretch.split(",")] + [0.0])
    subject = fit.deform(verts, synth.head_basis(verts), c_true)
    items, start = [], []
    for f in range(a.frames):
        pos, rot = training.rendered_pose(w, h, training.RENDER_SEED_BASE + f)
        R = render.euler_to_matrix(rot)
        items.append((f, 0, R, pos, 1.0, True))
        items.append((f, 1, np.eye(3), pos, 1.0, False))
        u = synth.SplitMix(31337 + f).uniform(6)
        d = 2.0 * u[:3] - 1.0
        R0 = render.euler_to_matrix(a.deg * (2.0 * u[3:] - 1.0)).astype(np.float64) @ R.astype(np.float64)
        start.append((f, 0, R0, pos + a.offset * d / np.sqrt((d * d).sum()), 1.0, False))
    inst = render.instances(start)

    def timed(call):
        meds = []
        for _ in range(a.runs):
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            meds.append(float(np.median(ms)))
        return {"ms": float(np.median(meds)), "min_run": min(meds), "max_run": max(meds)}

    with render.Mesh(subject, tris) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd, fit.Model.from_mesh(verts, tris) as model, fit.ShapeBasis(fields) as basis, fit.Fitter() as ft:
        frames, _ = rd.render([head, torso], render.instances(items), a.frames, w, h, K, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        torch.cuda.synchronize()
        fitted, frec = ft.fit(frames, [model], inst, K, device_out=True)
        t_fit = timed(lambda: ft.fit(frames, [model], inst, K, device_out=True))
        t_shape = timed(lambda: ft.shape_step(frames, model, basis, fitted, K, device_out=True))
        rec = ft.shape_step(frames, model, basis, fitted, K, device_out=True)
        torch.cuda.synchronize()
        rec = rec.cpu().numpy().view(_lib.SHAPE_RECORD_DTYPE)[0]
        frec = frec.cpu().numpy().view(_lib.FIT_RECORD_DTYPE)
        out = {"frames": a.frames, "size": a.size, "points": len(verts), "fields": a.fields, "fit": t_fit, "shape": t_shape,
               "shape_over_fit": t_shape["ms"] / t_fit["ms"], "fit_status_ok": int((frec["status"] == 0).sum()),
               "record": {"delta": rec["delta"][:a.fields].tolist(), "points": int(rec["points"]), "instances": int(rec["instances"]),
                          "status": int(rec["status"]), "rms_before": float(np.sqrt(int(rec["sum_r2_fixed"]) / 1048576.0 / max(int(rec["points"]), 1)))},
               "c_true": c_true[:a.fields].tolist()}
        if a.adapt > 0:
            host = frames[:a.adapt].cpu().view(torch.int16).numpy().view(np.uint16)
            c, _, trace = fit.adapt(ft, host, K, verts, tris, fields, inst[:a.adapt])
            out["adapt"] = {"frames": a.adapt, "coeffs": c.tolist(), "rms_by_round": [fit.rms(t["shape"]) for t in trace]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
