"""Multi-head tracking rate on one GPU: C cameras of 640 x 480 at stride 4, one frame per camera per step,
the bench forest, max_heads 4, r = 30.

For every C it reports
  * latency: one dh_multi_tracker_step_device followed by a stream synchronise, timed on the host clock (median of the steps);
  * rate:    cameras x steps / s of back-to-back steps with no host synchronisation, timed with device events;
each for direct calls and for replays of a captured step (dh_multi_tracker_capture + dh_graph_launch).  The yardstick in the
same process: dh_predict_heads_cameras_device on the same frames, latency and rate measured the same way.

    python tools/multi_track_rate.py [--cams 1,8,64,256] [--steps 50] [--warmup 5] [--repeats 3]

One JSON line per camera count.  For the kernel times run it under `rocprofv3 --kernel-trace --stats -- python ...` in a run of
its own.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cams", default="1,8,64,256")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--max-heads", type=int, default=4)
    ap.add_argument("--radius", type=int, default=30)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from track_rate import intrinsics, measure
    from depthhead_amd import synth
    from depthhead_amd.prediction import HoughPrediction
    from depthhead_amd.tracking import Cameras, MultiHeadTracker

    W, H, MH = args.width, args.height, args.max_heads
    forest = synth.fit_forest(10, 15, synth.FOREST_SEED_BASE + 2)          # bench.py's forest
    model = synth.ModelParams(stepwidth=args.stride)
    dev = torch.device("cuda:0")
    distinct = synth.biwi_batch(64, W, H)
    for C in [int(c) for c in args.cams.split(",")]:
        frames = torch.from_numpy(distinct[np.arange(C) % 64]).to(dev)
        n_heads = torch.zeros(C, dtype=torch.int32, device=dev)
        heads = torch.zeros(C * MH * 80, dtype=torch.uint8, device=dev)
        ids = torch.zeros(C * MH, dtype=torch.int32, device=dev)
        tracks = torch.zeros(C * 8 * 96, dtype=torch.uint8, device=dev)
        Ks = intrinsics(C, W, H)
        row = {"cams": C, "w": W, "h": H, "stride": args.stride, "max_heads": MH, "steps": args.steps, "repeats": args.repeats}
        with HoughPrediction(forest, model, device=0) as hp, Cameras(Ks) as cams:
            s = torch.cuda.current_stream().cuda_stream
            sync = torch.cuda.current_stream().synchronize
            hp.reserve(C, W, H)
            plain = lambda: hp.predict_heads_cameras_device(frames.data_ptr(), C, W, H, cams, n_heads.data_ptr(), heads.data_ptr(),
                                                            MH, args.radius, stream=s)
            row["heads_lat_us"], row["heads_rate"], row["heads_rates"] = measure(torch, plain, sync, args.steps, args.warmup, args.repeats, C)
            with MultiHeadTracker(hp, cams, W, H, MH, args.radius) as tr:
                direct = lambda: tr.step_device(frames.data_ptr(), n_heads.data_ptr(), heads.data_ptr(), ids.data_ptr(), stream=s)
                row["track_lat_us"], row["track_rate"], row["track_rates"] = measure(torch, direct, sync, args.steps, args.warmup, args.repeats, C)
                tr.reset()
                tr.capture(frames.data_ptr(), n_heads.data_ptr(), heads.data_ptr(), ids.data_ptr(), tracks.data_ptr())
                replay = lambda: hp.graph_launch(s)
                row["graph_lat_us"], row["graph_rate"], row["graph_rates"] = measure(torch, replay, sync, args.steps, args.warmup, args.repeats, C)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
