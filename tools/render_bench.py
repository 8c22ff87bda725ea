"""Time the renderer: `--frames` frames of `--size` with one head and one torso box each, rendered to device memory.
Prints one JSON line: frames/s over `--steps` renders (wall clock, after `--warmup`), and the device time of each kernel of
one profiled render (dh_renderer_set_profiling)."""
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
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--noise", type=int, default=2)
    ap.add_argument("--holes", type=float, default=0.02)
    a = ap.parse_args()
    import torch
    from depthhead_amd import render, synth, training
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    items = []
    for f in range(a.frames):
        pos, rot = training.rendered_pose(w, h, training.RENDER_SEED_BASE + f)
        items.append((f, 0, render.euler_to_matrix(rot), pos, 1.0, True))
        items.append((f, 1, np.eye(3), pos, 1.0, False))
    inst = render.instances(items)
    with render.Mesh(*synth.head_mesh()) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd:
        def once():
            return rd.render([head, torso], inst, a.frames, w, h, K, noise=a.noise, holes=a.holes, seed=1, device_out=True)
        for _ in range(a.warmup):
            once()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            once()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        rd.set_profiling(True)
        frames, masks = once()
        torch.cuda.synchronize()
        kern = rd.timing()
        fg = float((frames.view(torch.int16) != 0).float().mean())
    print(json.dumps({"frames": a.frames, "size": a.size, "render_ms": dt * 1e3, "frames_per_s": a.frames / dt,
                      "kernel_ms": kern, "kernels_total_ms": sum(kern.values()), "foreground": fg, "noise": a.noise, "holes": a.holes}))


if __name__ == "__main__":
    main()
