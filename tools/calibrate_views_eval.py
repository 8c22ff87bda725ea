"""Time one calibration step against the multi-view shape step over the same (person, view) pairs in the
same process: `--persons` heads (`synth.head_mesh(--subdiv)` and a torso box), each at a seeded world pose at the centre of its
own copy of ONE rig of `--views` cameras on an arc of +-35 degrees, persons * views device-resident frames of `--size`.  The
model is fitted once (dh_fit_depth_views_device); then, over the fitted poses:
  calib      dh_fit_calibrate_views_device on the table of persons * views cameras, one set: every camera's row takes ONE pair;
  calib_sets the same call on the table of the one rig's `--views` cameras with person p as set p -- the same frames in the
             same memory, but `--persons` pairs land in each of `--views` rows: the contended case;
  shape      the yardstick, dh_fit_shape_views_device on the table of persons * views cameras with the first `--fields` fields of
             `synth.head_basis`, all in one subject: the same point passes, one row.
The three calls alternate, run after run.  Prints one JSON line: ms per call measured with device events around each of
`--steps` calls (after `--warmup`), as the median over the calls of each of `--runs` repeats and the spread of those medians,
the ratios, and what the calibration records say."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--persons", type=int, default=64)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--fields", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--offset", type=float, default=15.0)
    ap.add_argument("--deg", type=float, default=6.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import _lib, fit, render, synth
    from depthhead_amd.tracking import Cameras
    w, h = (int(v) for v in a.size.split("x"))
    n = a.persons * a.views
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    fields = synth.head_basis(verts)[:a.fields]
    yaws = np.linspace(-35.0, 35.0, a.views) if a.views > 1 else np.zeros(1)
    dist = 700.0 + 500.0 * synth.SplitMix(53000).uniform(a.views)
    rig_R, rig_t = [], []
    for k in range(a.views):
        ca, sa = np.cos(np.radians(yaws[k])), np.sin(np.radians(yaws[k]))
        Rc = np.array([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]])
        rig_R.append(Rc)
        rig_t.append(-dist[k] * Rc[:, 2])
    V1, u1 = fit.views_from_rig(np.array(rig_R), np.array(rig_t))               # the one rig
    V, uu = np.tile(V1, (a.persons, 1, 1)), np.tile(u1, (a.persons, 1))         # and its copy per person
    items, start = [], np.zeros(a.persons, _lib.VIEW_INSTANCE_DTYPE)
    for p in range(a.persons):
        u = synth.SplitMix(52000 + p).uniform(12)
        pos = 60.0 * (2.0 * u[:3] - 1.0)
        R = render.euler_to_matrix(np.array([30.0, 15.0, 10.0]) * (2.0 * u[3:6] - 1.0)).astype(np.float64)
        d = 2.0 * u[6:9] - 1.0
        R0 = render.euler_to_matrix(a.deg * (2.0 * u[9:12] - 1.0)).astype(np.float64) @ R
        start[p] = (p * a.views, 0, (1 << a.views) - 1, R0.astype(np.float32).reshape(9), (pos + a.offset * d / np.sqrt((d * d).sum())).astype(np.float32),
                    1.0, 0)
        for k in range(a.views):
            Vc, uc = V1[k].astype(np.float64), u1[k].astype(np.float64)
            items += [(p * a.views + k, 0, Vc @ R, Vc @ pos + uc, 1.0, True), (p * a.views + k, 1, Vc, Vc @ pos + uc, 1.0, False)]

    def run(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()

    with render.Mesh(verts, tris) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd, fit.Model.from_mesh(verts, tris) as model, fit.ShapeBasis(fields) as basis, fit.Fitter() as ft, \
            Cameras(np.tile(K.reshape(1, 9), (n, 1))) as cams, fit.Views(cams, V, uu) as views, \
            Cameras(np.tile(K.reshape(1, 9), (a.views, 1))) as cams1, fit.Views(cams1, V1, u1) as views1:
        frames, _ = rd.render([head, torso], render.instances(items), n, w, h, cams, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        d_fit, d_frec = ft.fit_views(frames, [model], start, views, device_out=True)
        torch.cuda.synchronize()
        fitted = d_fit.cpu().numpy().view(_lib.VIEW_INSTANCE_DTYPE).copy()
        frec = d_frec.cpu().numpy().view(_lib.VIEW_FIT_RECORD_DTYPE)
        by_set = fitted.copy()
        by_set["first_cam"] = 0
        d_by_set, d_sets = dev(by_set), torch.arange(a.persons, dtype=torch.int32, device="cuda")
        one_set, many_sets = frames.view(1, n, h, w), frames.view(a.persons, a.views, h, w)
        calls = {"calib": lambda: ft.calibrate_step(one_set, views, model, d_fit, device_out=True),
                 "calib_sets": lambda: ft.calibrate_step(many_sets, views1, model, d_by_set, sets=d_sets, device_out=True),
                 "shape": lambda: ft.shape_step_views(one_set, views, model, basis, d_fit, device_out=True)}
        meds = {name: [] for name in calls}
        for _ in range(a.runs):                                       # alternating, run after run
            for name in ("shape", "calib", "calib_sets"):
                meds[name].append(run(calls[name]))
        recs = {}
        for name in ("calib", "calib_sets"):
            r = calls[name]()
            torch.cuda.synchronize()
            recs[name] = r.cpu().numpy().view(_lib.CALIB_RECORD_DTYPE).copy()

    def stat(v):
        return {"ms": float(np.median(v)), "min_run": min(v), "max_run": max(v)}

    def records(r):
        ok = r["status"] == 0
        rms = np.sqrt(r["sum_r2_fixed"][ok] / 1048576.0 / np.maximum(r["points"][ok], 1))
        return {"cameras": len(r), "ok": int(ok.sum()), "points": int(r["points"].sum()), "pairs": int(r["pairs"].sum()),
                "rms_before": float(np.median(rms)) if ok.any() else None,
                "largest_d_mm": float(np.abs(r["delta"][:, :3]).max()), "largest_w_deg": float(np.degrees(np.abs(r["delta"][:, 3:]).max()))}

    print(json.dumps({"persons": a.persons, "views": a.views, "cameras": n, "size": a.size, "points": len(verts), "fields": a.fields,
                      "workgroups": {"calib": a.persons * min(64, n), "calib_sets": a.persons * min(64, a.views), "shape": a.persons * min(64, n)},
                      "calibrate_views": stat(meds["calib"]), "calibrate_views_sets": stat(meds["calib_sets"]), "shape_views": stat(meds["shape"]),
                      "calib_over_shape": float(np.median(meds["calib"]) / np.median(meds["shape"])),
                      "calib_sets_over_shape": float(np.median(meds["calib_sets"]) / np.median(meds["shape"])),
                      "fit_status_ok": int((frec["status"] == 0).sum()),
                      "records": records(recs["calib"]), "records_sets": records(recs["calib_sets"])}))


if __name__ == "__main__":
    main()
