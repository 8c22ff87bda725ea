"""Does the fit repair the forest's poses?  The protocol of DESIGN.md section 17 (tests/test_gpu_render_pipeline.py): a forest
trained on 160 rendered frames of 320x240 predicts 48 held-out rendered frames; each predicted pose then starts a fit of the head
model against its frame.  Prints one JSON line: position error (mean / max, mm), mean absolute yaw error and mean geodesic
rotation error (degrees) before and after, the fit's exit statuses, and the same for each coarse gate of `--gates` (the default
parameters are the first entry; nothing here is fed back into them)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 320, 240
N_TRAIN, N_TEST, TEST_FIRST = 160, 48, 100000
LEARN = (8, 80, 80, 10, 6, 3000, 0.3, 200, 20, 5.0)
SEED, SIGMA, PREDICT_STEP = 17, 8.0, 4


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gates", default="120,160,200,300", help="coarse gates (mm) to report; the first is the default")
    a = ap.parse_args()
    from depthhead_amd import fit, render, synth, training
    from depthhead_amd.prediction import HoughPrediction, IntrinsicMatrix
    train = list(training.rendered_data(N_TRAIN, W, H, first=0))
    test = list(training.rendered_data(N_TEST, W, H, first=TEST_FIRST))
    forest, model = training.HoughLearning(*LEARN, seed=SEED).learn(SIGMA, iter(train))
    model.stepwidth = PREDICT_STEP
    frames = np.stack([t[0] for t in test])
    K = test[0][2]
    with HoughPrediction(forest, model, device=0) as hp:
        poses = hp.predict_batch(frames, IntrinsicMatrix(K))
    truth_pos = np.stack([t[3] for t in test]).astype(np.float64)
    truth_rot = np.stack([t[4] for t in test]).astype(np.float64)
    truth_R = [render.euler_to_matrix(r).astype(np.float64) for r in truth_rot]
    start = fit.instances_from_poses(poses)

    def report(inst):
        pos = np.sqrt(((inst["t"].astype(np.float64) - truth_pos) ** 2).sum(axis=1))
        eul = np.stack([fit.matrix_to_euler(r.reshape(3, 3)) for r in inst["R"]])
        geo = [np.degrees(np.arccos(np.clip((np.trace(truth_R[i].T @ inst["R"][i].reshape(3, 3).astype(np.float64)) - 1.0) / 2.0, -1, 1)))
               for i in range(len(inst))]
        return {"pos_mean_mm": float(pos.mean()), "pos_max_mm": float(pos.max()), "pos_median_mm": float(np.median(pos)),
                "within_10mm": int((pos <= 10.0).sum()),
                "yaw_abs_deg": float(np.abs(eul[:, training.YAW] - truth_rot[:, training.YAW]).mean()), "geodesic_deg": float(np.mean(geo))}

    out = {"frames": N_TEST, "nodes": forest.n_nodes, "forest": report(start),
           "yaw_const_deg": float(np.abs(np.mean([t[4][training.YAW] for t in train]) - truth_rot[:, training.YAW]).mean()), "fit": {}}
    verts, tris = synth.head_mesh()
    with fit.Model.from_mesh(verts, tris) as m, fit.Fitter() as ft:
        for g in (float(v) for v in a.gates.split(",")):
            got, rec = ft.fit(frames, [m], start, K, params=fit.fit_params(gate=(g, 25.0)))
            r = report(got)
            r.update({"status": np.bincount(rec["status"], minlength=3).tolist(), "points_mean": float(rec["points"].mean()),
                      "rms_mean_mm": float(np.nanmean([fit.rms(x) for x in rec]))})
            out["fit"][f"gate {g:g}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
