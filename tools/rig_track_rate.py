"""Rig tracking rate on one GPU: C cameras of 640 x 480 at stride 4 in rigs of --rig-size cameras, one
frame per camera per step, the bench forest, max_heads 4, r = 30.  The cameras of a rig stand 25 mm apart along x, so that
views of one head fuse.

For every C it reports latency (one call followed by a stream synchronise, host clock, median of the steps) and rate (cameras x
steps / s of back-to-back calls with no host synchronisation, device events) of
  * heads:  dh_predict_heads_cameras_device        (the yardstick),
  * multi:  dh_multi_tracker_step_device           (section 15),
  * rig:    dh_rig_tracker_step_device, and replays of a captured rig step (graph),
measured in turns in the same process: --repeats rounds of heads, multi, rig, graph; the medians over the rounds are reported
beside every round's figure.

    python tools/rig_track_rate.py [--cams 1,8,64,256] [--rig-size 4] [--steps 50] [--warmup 5] [--repeats 3]

One JSON line per camera count.  For k_rig_fuse's own time run it under `rocprofv3 --kernel-trace --stats -- python ...` in a
run of its own.
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
    ap.add_argument("--rig-size", type=int, default=4)
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
    from depthhead_amd.tracking import Cameras, MultiHeadTracker, Rig, RigTracker

    W, H, MH = args.width, args.height, args.max_heads
    forest = synth.fit_forest(10, 15, synth.FOREST_SEED_BASE + 2)          # bench.py's forest
    model = synth.ModelParams(stepwidth=args.stride)
    dev = torch.device("cuda:0")
    distinct = synth.biwi_batch(64, W, H)
    for C in [int(c) for c in args.cams.split(",")]:
        size = min(args.rig_size, C)
        rig_begin = list(range(0, C, size)) + [C]
        ng = len(rig_begin) - 1
        # the cameras of a rig see the rig's frame
        frames = torch.from_numpy(distinct[(np.arange(C) // size) % 64]).to(dev)
        z = lambda count, dt: torch.zeros(count, dtype=dt, device=dev)   # noqa: E731
        n_heads, heads, ids = z(C, torch.int32), z(C * MH * 80, torch.uint8), z(C * MH, torch.int32)
        n_persons, persons, tracks = z(ng, torch.int32), z(ng * 16 * 56, torch.uint8), z(ng * 16 * 72, torch.uint8)
        R = np.tile(np.eye(3, dtype=np.float32).reshape(9), (C, 1))
        t = np.zeros((C, 3), dtype=np.float32)
        t[:, 0] = (np.arange(C) % size) * 25 % 100
        row = {"cams": C, "rig_size": size, "rigs": ng, "w": W, "h": H, "stride": args.stride, "max_heads": MH, "steps": args.steps,
               "repeats": args.repeats}
        with HoughPrediction(forest, model, device=0) as hp, Cameras(intrinsics(C, W, H)) as cams, Rig(cams, R, t, rig_begin) as rig:
            s = torch.cuda.current_stream().cuda_stream
            sync = torch.cuda.current_stream().synchronize
            hp.reserve(C, W, H)
            with MultiHeadTracker(hp, cams, W, H, MH, args.radius) as mt, RigTracker(hp, rig, W, H, MH, args.radius) as rt, \
                    RigTracker(hp, rig, W, H, MH, args.radius) as rg:
                rig_args = (frames.data_ptr(), n_heads.data_ptr(), heads.data_ptr(), ids.data_ptr(), n_persons.data_ptr(), persons.data_ptr())
                rg.capture(*rig_args, tracks_ptr=tracks.data_ptr())
                calls = {
                    "heads": lambda: hp.predict_heads_cameras_device(frames.data_ptr(), C, W, H, cams, n_heads.data_ptr(), heads.data_ptr(),
                                                                     MH, args.radius, stream=s),
                    "multi": lambda: mt.step_device(frames.data_ptr(), n_heads.data_ptr(), heads.data_ptr(), ids.data_ptr(), stream=s),
                    "rig": lambda: rt.step_device(*rig_args, stream=s),
                    "graph": lambda: hp.graph_launch(s),
                }
                rounds = {k: [] for k in calls}
                for _ in range(args.repeats):
                    for k, fn in calls.items():
                        lat, rate, _ = measure(torch, fn, sync, args.steps, args.warmup, 1, C)
                        rounds[k].append((lat, rate))
                for k, v in rounds.items():
                    row[k + "_lat_us"] = float(np.median([x[0] for x in v]))
                    row[k + "_rate"] = float(np.median([x[1] for x in v]))
                    row[k + "_rounds"] = [[round(float(x[0]), 1), round(float(x[1]), 1)] for x in v]
                sync()
                row["persons_last_step"] = int(n_persons.sum().item())
                row["max_views"] = int(persons.cpu().numpy().view(np.uint32).reshape(-1, 14)[:, 7].max())
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
