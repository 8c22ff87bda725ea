"""Cost of the vote-support calls on the bench workload: 256 frames of 640 x 480, stride 4, the fitted 10-tree forest, device
batches with `--inflight` batches queued per step, plain and support calls alternating in one process; then one frame at a
time with a host sync.  Prints one JSON line per configuration.

    python tools/support_rate.py [--frames 256] [--rounds 5] [--steps 8] [--inflight 4] [--radius 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

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
    sups = [torch.zeros(n * 40, dtype=torch.uint8, device=dev) for _ in range(q)]
    with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp:
        s = torch.cuda.current_stream().cuda_stream

        def step(sup):
            for j in range(q):
                if sup:
                    hp.predict_batch_support_device(frames.data_ptr(), n, W, H, K, outs[j].data_ptr(), sups[j].data_ptr(), radius, stream=s)
                else:
                    hp.predict_batch_device(frames.data_ptr(), n, W, H, K, outs[j].data_ptr(), stream=s)

        for sup in (False, True):      # warm-up (the first support call allocates its scratch)
            step(sup)
        torch.cuda.synchronize()
        res = {False: [], True: []}
        for _ in range(args.rounds):
            for sup in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    step(sup)
                e1.record()
                torch.cuda.synchronize()
                res[sup].append(e0.elapsed_time(e1) / args.steps)
        for sup in (False, True):
            ms = res[sup]
            print(json.dumps({"config": f"{n} frames x {q} in flight", "support": sup, "step_ms": ms,
                              "median_step_ms": float(np.median(ms)), "frames_per_s": float(n * q / (np.median(ms) / 1e3))}))
        # one frame at a time, host sync after each
        one = synth.biwi_batch(1, W, H)
        lat = {False: [], True: []}
        for _ in range(3):
            hp.predict_batch(one, K); hp.predict_batch_support(one, K, radius)
        for _ in range(args.rounds * 8):
            for sup in (False, True):
                t0 = time.perf_counter()
                if sup:
                    hp.predict_batch_support(one, K, radius)
                else:
                    hp.predict_batch(one, K)
                lat[sup].append((time.perf_counter() - t0) * 1e3)
        for sup in (False, True):
            print(json.dumps({"config": "1 frame, host call", "support": sup, "median_ms": float(np.median(lat[sup])),
                              "p10_ms": float(np.percentile(lat[sup], 10)), "p90_ms": float(np.percentile(lat[sup], 90))}))


if __name__ == "__main__":
    main()
