"""Train a Hough forest on the GPU: the reference's examples/hough_tree_trainer.rs.

    python tools/train_forest.py --synthetic 2000 --out forest.npz --json forest.json
    python tools/train_forest.py --biwi /data/biwi --persons 1-20 --out forest.npz
    python tools/train_forest.py --synthetic 2000 --bench      # one JSON line of timings

Defaults are the trainer binary's: depth 15, 5200 samples per tree, 2000 features per node, steepness 5.0, 20 trees,
min subset 20, stepwidth 10, 80 x 80 patches, rectangle factor 0.3.  Writes a `Forest.save` file and `export_json`.
--bench also fits a reduced configuration with the C oracle of the test suite (tests/train_ref) and on the GPU."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from depthhead_amd import synth, training  # noqa: E402
from depthhead_amd.stamm_json import export_json  # noqa: E402


def persons(spec: str):
    out = []
    for part in spec.split(","):
        a, _, b = part.partition("-")
        out.extend(range(int(a), int(b or a) + 1))
    return out


def synthetic_batches(n, w, h, batch=64):
    for b0 in range(0, n, batch):
        items = [training.synthetic_truth(w, h, synth.FRAME_SEED_BASE + i) for i in range(b0, min(n, b0 + batch))]
        fr, ma, K, p3, rd = zip(*items)
        yield np.stack(fr), np.stack(ma), np.stack([k.reshape(9) for k in K]), np.stack(p3), np.stack(rd)


def oracle_reduced(args):
    """The reduced configuration fitted by the C oracle and by the GPU: (config, oracle s, gpu s, equal, verifier gap)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "train_ref"))
    import train_util as tu
    cfg = dict(stepwidth=args.stepwidth, W=args.width, H=args.height, max_depth=args.depth, n_trees=2, subset=args.subset,
               scale=args.scale, F=200, min_subset=args.min_subset, steep=args.steepness, seed=args.seed)
    p = tu.params(**cfg)
    data = tu.synthetic(48, args.frame_w, args.frame_h)
    t0 = time.perf_counter()
    ref, _, _ = tu.oracle_train(p, [data])
    t_or = time.perf_counter() - t0
    with training.Trainer(p) as tr:
        tr.add_frames(*data)
        t0 = time.perf_counter()
        got = tr.fit()
        t_gpu = time.perf_counter() - t0
    cfg.update(frames=48, frame=f"{args.frame_w}x{args.frame_h}")
    gap = tu.oracle_verify(p, got)[0]        # raises if the GPU forest fails the node-by-node check
    return cfg, t_or, t_gpu, tu.forest_equal(got, ref), gap


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--biwi", help="BIWI Kinect Head Pose directory (db_reader layout)")
    src.add_argument("--synthetic", type=int, help="N synthetic frames (depthhead_amd.training.synthetic_truth)")
    ap.add_argument("--persons", default="1-24", help="BIWI persons, e.g. 1-20,22")
    ap.add_argument("--frame-w", type=int, default=640)
    ap.add_argument("--frame-h", type=int, default=480)
    ap.add_argument("--depth", type=int, default=15)
    ap.add_argument("--subset", type=int, default=5200)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--steepness", type=float, default=5.0)
    ap.add_argument("--trees", type=int, default=20)
    ap.add_argument("--min-subset", type=int, default=20)
    ap.add_argument("--stepwidth", type=int, default=10)
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--scale", type=float, default=0.3)
    ap.add_argument("--sigma", type=float, default=8.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", help="Forest.save output (.npz)")
    ap.add_argument("--json", help="export_json output")
    ap.add_argument("--bench", action="store_true", help="print one JSON line of timings")
    args = ap.parse_args()

    hl = training.HoughLearning(args.stepwidth, args.width, args.height, args.depth, args.trees, args.subset, args.scale,
                                args.features, args.min_subset, args.steepness, seed=args.seed, device=args.device)
    if args.biwi:
        from depthhead_amd.biwi import BiwiReader
        reader = BiwiReader(os.path.join(args.biwi, "head_pose_masks"), os.path.join(args.biwi, "hpdb"),
                            os.path.join(args.biwi, "db_annotations"))
        t0 = time.perf_counter()
        forest, model = hl.learn_biwi(args.sigma, reader, persons(args.persons))
        t_all = time.perf_counter() - t0
        st, t_ingest, t_fit = hl.last_stats, None, None
    else:
        with hl.trainer() as tr:
            t_ingest = 0.0
            for batch in synthetic_batches(args.synthetic, args.frame_w, args.frame_h):
                t0 = time.perf_counter()
                tr.add_frames(*batch)
                t_ingest += time.perf_counter() - t0
            t0 = time.perf_counter()
            forest = tr.fit()
            t_fit = time.perf_counter() - t0
            st = tr.stats()
        model = synth.ModelParams(args.stepwidth, args.width, args.height, args.sigma, 20)
        t_all = None
    if args.out:
        forest.save(args.out)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(export_json(forest, model))
    if args.bench:
        cfg, t_or, t_gpu, equal, gap = oracle_reduced(args)
        print(json.dumps({"frames": st["frames"], "pool": st["pool_size"], "pool_positives": st["pool_positives"],
                          "ingest_s": t_ingest, "fit_s": t_fit, "learn_s": t_all, "level_ms": [round(x, 3) for x in st["level_ms"]],
                          "nodes": forest.n_nodes, "leaves": forest.n_leaves, "max_depth": forest.max_depth(),
                          "neg_det": st["neg_det"], "reduced": cfg, "reduced_oracle_fit_s": t_or, "reduced_gpu_fit_s": t_gpu,
                          "reduced_equal": equal, "reduced_verified": True, "reduced_gap": gap}))
    else:
        print(f"{forest.n_trees} trees, {forest.n_nodes} split nodes, {forest.n_leaves} leaves, depth {forest.max_depth()} "
              f"from {st['pool_size']} samples ({st['pool_positives']} positive)")


if __name__ == "__main__":
    main()
