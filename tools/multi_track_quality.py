"""Candidate scenes for the multi-head tracker's quality test (tests/test_gpu_multi_track_quality.py).

Each candidate is one camera of a single tracker: two synthetic heads in a 320 x 240 scene, the second moving 2 pixels per step
for 12 steps, the 6-tree test forest at stride 4.  One JSON line per candidate: the worst distance from a true head to its
nearest detected head, whether the two nearest heads were always distinct, and whether their ids held.

    python tools/multi_track_quality.py [--first 0] [--count 16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--count", type=int, default=16)
    args = ap.parse_args()
    import test_gpu_multi_track_quality as q
    from depthhead_amd import prediction, synth, tracking
    firsts = list(range(args.first, args.first + args.count))
    forest = synth.fit_forest(*q.FOREST_ARGS, n_frames=12, subset=1500)
    frames, truths = q.scenes(firsts)
    K = synth.default_intrinsic(q.W, q.H)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, \
            tracking.Cameras(np.repeat(K[None], len(firsts), 0)) as cams:
        worst, distinct, ids, held = q.evaluate(hp, tracking, cams, frames, truths)
    for i, f in enumerate(firsts):
        print(json.dumps({"first": f, "worst_mm": round(float(worst[i]), 1), "distinct": bool(distinct[i]), "ids_held": held[i],
                          "ids": ids[:, i].tolist()}), flush=True)


if __name__ == "__main__":
    main()
