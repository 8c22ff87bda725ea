"""Cost of the several-heads calls on the bench workload: 256 frames of 640 x 480, stride 4, the fitted 10-tree forest, device
batches with `--inflight` batches queued per step; the plain step, then heads steps at max_heads 1 and 4, alternating in one
process.  Prints one JSON line per configuration.

    python tools/heads_rate.py [--frames 256] [--rounds 5] [--steps 8] [--inflight 4] [--radius 30]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--radius", type=int, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from depthhead_amd import _lib, synth
    from depthhead_amd.prediction import HoughPrediction, IntrinsicMatrix
    radius = _lib.SUPPORT_RADIUS if args.radius is None else args.radius
    W, H, n = 640, 480, args.frames
    forest = synth.fit_forest(10, 15, synth.FOREST_SEED_BASE + 2)
    K = IntrinsicMatrix(synth.default_intrinsic(W, H))
    dev = torch.device("cuda", 0)
    frames = torch.from_numpy(synth.biwi_batch(n, W, H)).to(dev)
    q = args.inflight
    outs = [torch.zeros(n * 40, dtype=torch.uint8, device=dev) for _ in range(q)]
    nhs = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(q)]
    heads = [torch.zeros(n * _lib.MAX_HEADS * 80, dtype=torch.uint8, device=dev) for _ in range(q)]
    configs = (0, 1, _lib.MAX_HEADS)         # 0: the plain step
    with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp:
        s = torch.cuda.current_stream().cuda_stream

        def step(mh):
            for j in range(q):
                if mh:
                    hp.predict_heads_device(frames.data_ptr(), n, W, H, K, nhs[j].data_ptr(), heads[j].data_ptr(), mh, radius, stream=s)
                else:
                    hp.predict_batch_device(frames.data_ptr(), n, W, H, K, outs[j].data_ptr(), stream=s)

        for mh in configs:                  # warm-up (the first heads call allocates its scratch)
            step(mh)
        torch.cuda.synchronize()
        res = {mh: [] for mh in configs}
        for _ in range(args.rounds):
            for mh in configs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    step(mh)
                e1.record()
                torch.cuda.synchronize()
                res[mh].append(e0.elapsed_time(e1) / args.steps)
        plain = float(np.median(res[0]))
        for mh in configs:
            ms = float(np.median(res[mh]))
            print(json.dumps({"config": f"{n} frames x {q} in flight", "max_heads": mh, "step_ms": res[mh], "median_step_ms": ms,
                              "frames_per_s": n * q / (ms / 1e3), "vs_plain": ms / plain}))
        nh = nhs[0].cpu().numpy()
        print(json.dumps({"n_heads_histogram": np.bincount(nh, minlength=_lib.MAX_HEADS + 1).tolist()}))


if __name__ == "__main__":
    main()
