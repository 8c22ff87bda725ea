"""Candidate scenes for the rig tracker's quality test (tests/test_gpu_rig_quality.py).

Each candidate is one rig of two cameras with parallel axes: camera A sees section 15's two-head scene, camera B the same frame
moved by an integer disparity.  With --cpu (no GPU needed) the heads come from the CPU restatement (tests/heads_ref.py on the C
oracle's taps) and the persons from tests/rig_track_ref.py; without it, from the GPU's RigTracker.  One JSON line per
candidate: whether both true heads are found in both views at every step (the criterion that keeps a scene), whether every step
has two persons with the expected views, whether their ids hold, the worst Chebyshev distance of a person's cell from the true
world position, and the worst single-view distance of the same heads (cell of the head's world midpoint against the truth).

    python tools/rig_track_quality.py --cpu [--first 0] [--count 24]
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


def cpu_heads(frames, K, forest, model, q):
    """(n_heads [steps, cams], heads [steps, cams, max_heads]) from the CPU restatement of the heads pipeline"""
    import heads_ref as hr
    import support_ref as sr
    from depthhead_amd._lib import HEAD_DTYPE
    from oracle import pyoracle
    pyoracle.lib()
    tab = sr.LeafTables(forest)
    steps, cams = frames.shape[:2]
    n_heads = np.zeros((steps, cams), dtype=np.uint32)
    heads = np.zeros((steps, cams, q.MAX_HEADS), dtype=HEAD_DTYPE)
    for k in range(steps):
        for c in range(cams):
            n, kept, _, _, _ = hr.heads_ref(pyoracle, tab, model, frames[k, c], K, q.MAX_HEADS, q.RADIUS)
            n_heads[k, c] = n
            heads[k, c] = hr.as_records(n, kept, q.MAX_HEADS, HEAD_DTYPE)
    return n_heads, heads


def found(n_heads, heads, t, truths, q):
    """Both true heads found in both views at every step; and the worst single-view distances (Euclidean of the midpoint as
    sections 14 / 15 measure it, Chebyshev of the world cell as the persons are measured)"""
    ok, worst_e, worst_c = True, 0.0, 0.0
    for k in range(q.STEPS):
        for v in range(2):
            if n_heads[k, v] != 2:
                return False, np.inf, np.inf
            mids = heads[k, v, :2]["pose"]["mid_point"].astype(np.float64) + t[v].astype(np.float64)
            near = []
            for h in range(2):
                d = np.linalg.norm(mids - truths[k, h], axis=1)
                j = int(np.argmin(d))
                near.append(j)
                worst_e = max(worst_e, float(d[j]))
                worst_c = max(worst_c, float(np.abs(np.trunc(mids[j]) - truths[k, h]).max()))
            ok = ok and near[0] != near[1]
    return ok and worst_e <= q.FOUND_MM, worst_e, worst_c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--count", type=int, default=24)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    import rig_track_ref as rr
    import test_gpu_rig_quality as q
    from depthhead_amd import _lib, synth
    firsts = list(range(args.first, args.first + args.count))
    forest = synth.fit_forest(*q.FOREST_ARGS, n_frames=12, subset=1500)
    model = synth.ModelParams(stepwidth=4)
    K = synth.default_intrinsic(q.W, q.H)
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1))
    for f in firsts:
        frames, truths, t = q.two_views([f])
        present = q.presence(1)
        if args.cpu:
            n_heads, heads = cpu_heads(frames, K, forest, model, q)
            ref = rr.Restatement(eye, t, [0, 2], q.MAX_HEADS, _lib.RIG_FUSE_GATE, _lib.TRACK_GATE, _lib.TRACK_MAX_MISSES,
                                 _lib.RIG_TRACK_DTYPE, _lib.RIG_PERSON_DTYPE)
            outs = [ref.step(n_heads[k], heads[k], present[k]) for k in range(q.STEPS)]
            n_persons, persons = [o[1][0] for o in outs], [o[2][0] for o in outs]
        else:
            from depthhead_amd import prediction, tracking
            with prediction.HoughPrediction(forest, model) as hp, tracking.Cameras(np.repeat(K[None], 2, 0)) as cams, \
                    q.rig_of(tracking, cams, t, 1) as rig, tracking.RigTracker(hp, rig, q.W, q.H, q.MAX_HEADS, q.RADIUS) as tr:
                outs = [tr.step(frames[k], present[k]) for k in range(q.STEPS)]
                n_heads, heads = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
            n_persons, persons = [o[3][0] for o in outs], [o[4][0] for o in outs]
        ok, single_e, single_c = found(n_heads, heads, t, truths[:, 0], q)
        res = q.judge(n_persons, persons, present, truths[:, 0])
        print(json.dumps({"first": f, "found": bool(ok), "single_view_worst_mm": round(single_e, 1),
                          "single_view_worst_cheb_mm": round(single_c, 1), "two_persons": bool(res["two_persons"]),
                          "views_ok": bool(res["views_ok"]), "ids_held": res["ids_held"],
                          "fused_worst_cheb_mm": round(float(res["worst_mm"]), 1), "ids": res["ids"].tolist()}), flush=True)


if __name__ == "__main__":
    main()
