"""Live tracking rate on one GPU: C cameras of 640 x 480 at stride 4, one frame per camera per step.

For every C it reports
  * latency: one dh_tracker_step_device followed by a stream synchronise, timed on the host clock (median of the steps);
  * rate:    cameras x steps / s of back-to-back steps with no host synchronisation, timed with device events;
each for direct calls and for replays of a captured step (dh_tracker_capture + dh_graph_launch).  The yardsticks in the same
process: the plain device batch (dh_predict_batch_device) of C frames with one K, latency and rate measured the same way.

    python tools/track_rate.py [--cams 1,8,64,256] [--steps 200] [--warmup 20] [--repeats 3]

One JSON line per camera count.  For the kernel times run it under `rocprofv3 --kernel-trace --stats -- python ...` in a run of
its own.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def intrinsics(n, w, h):
    from depthhead_amd import synth
    K0 = synth.default_intrinsic(w, h).astype(np.float32)
    ks = np.repeat(K0[None], n, 0)
    for c in range(n):                          # every camera its own calibration (pinhole)
        ks[c, 0, 0] *= 1.0 + 0.004 * (c % 11); ks[c, 1, 1] *= 1.0 + 0.003 * (c % 7)
        ks[c, 0, 2] += (c % 5) - 2.0; ks[c, 1, 2] += (c % 3) - 1.0
    return ks


def measure(torch, step, sync, steps, warmup, repeats, per_step):
    """(median latency with a synchronise per step in us, rate in items / s without one)"""
    for _ in range(warmup):
        step()
    sync()
    lat = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        sync()
        lat.append(time.perf_counter() - t0)
    rates = []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(repeats):
        ev0.record()
        for _ in range(steps):
            step()
        ev1.record()
        ev1.synchronize()
        rates.append(per_step * steps / (ev0.elapsed_time(ev1) * 1e-3))
    return float(np.median(lat) * 1e6), float(np.median(rates)), [round(r, 1) for r in rates]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cams", default="1,8,64,256")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from depthhead_amd import synth
    from depthhead_amd.prediction import HoughPrediction, IntrinsicMatrix
    from depthhead_amd.tracking import Cameras, HeadTracker

    W, H = args.width, args.height
    forest = synth.fit_forest(10, 15, synth.FOREST_SEED_BASE + 2)          # bench.py's forest
    model = synth.ModelParams(stepwidth=args.stride)
    dev = torch.device("cuda:0")
    distinct = synth.biwi_batch(64, W, H)
    for C in [int(c) for c in args.cams.split(",")]:
        frames = torch.from_numpy(distinct[np.arange(C) % 64]).to(dev)
        out = torch.zeros(C * 40, dtype=torch.uint8, device=dev)
        Ks = intrinsics(C, W, H)
        row = {"cams": C, "w": W, "h": H, "stride": args.stride, "steps": args.steps, "repeats": args.repeats}
        with HoughPrediction(forest, model, device=0) as hp, Cameras(Ks) as cams:
            s = torch.cuda.current_stream().cuda_stream
            sync = torch.cuda.current_stream().synchronize
            K = IntrinsicMatrix(Ks[0])
            hp.reserve(C, W, H)
            plain = lambda: hp.predict_batch_device(frames.data_ptr(), C, W, H, K, out.data_ptr(), stream=s)
            row["batch_lat_us"], row["batch_rate"], row["batch_rates"] = measure(torch, plain, sync, args.steps, args.warmup, args.repeats, C)
            with HeadTracker(hp, cams, W, H, prev_guess=True, sluggish=True) as tr:
                direct = lambda: tr.step_device(frames.data_ptr(), out.data_ptr(), stream=s)
                row["track_lat_us"], row["track_rate"], row["track_rates"] = measure(torch, direct, sync, args.steps, args.warmup, args.repeats, C)
                tr.reset()
                tr.capture(frames.data_ptr(), out.data_ptr())
                replay = lambda: hp.graph_launch(s)
                row["graph_lat_us"], row["graph_rate"], row["graph_rates"] = measure(torch, replay, sync, args.steps, args.warmup, args.repeats, C)
            hp.graph_capture(frames.data_ptr(), C, W, H, K, out.data_ptr())
            replay = lambda: hp.graph_launch(s)
            row["batch_graph_lat_us"], row["batch_graph_rate"], row["batch_graph_rates"] = measure(torch, replay, sync, args.steps, args.warmup, args.repeats, C)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
