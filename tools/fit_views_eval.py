"""Time the multi-view fit against the single-view fit of the same frames in the same process:
`--persons` heads (`synth.head_mesh(--subdiv)` and a torso box), each at a seeded world pose and seen by `--views` cameras on an
arc of +-35 degrees about it, persons * views device-resident frames of `--size`.  dh_fit_depth_views_device fits one world
pose per person against all its views; the yardstick, dh_fit_depth_cameras_device, fits one instance per frame through that
frame's camera.  Both start `--offset` mm and up to `--deg` degrees per axis from the truth.  The two calls alternate, run after
run.  Prints one JSON line: ms per call measured with device events around each of `--steps` calls (after `--warmup`), as the
median over the calls of each of `--runs` repeats and the spread of those medians, for both, and the mean position and
rotation errors of both."""
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--offset", type=float, default=60.0)
    ap.add_argument("--deg", type=float, default=15.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import _lib, fit, render, synth
    from depthhead_amd.tracking import Cameras
    w, h = (int(v) for v in a.size.split("x"))
    n = a.persons * a.views
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    yaws = np.linspace(-35.0, 35.0, a.views) if a.views > 1 else np.zeros(1)
    rig_R, rig_t, items, multi, single, truth = [], [], [], [], [], []
    for p in range(a.persons):
        u = synth.SplitMix(52000 + p).uniform(12 + a.views)
        pos = 60.0 * (2.0 * u[:3] - 1.0)
        R = render.euler_to_matrix(np.array([30.0, 15.0, 10.0]) * (2.0 * u[3:6] - 1.0)).astype(np.float64)
        d = 2.0 * u[6:9] - 1.0
        R0 = render.euler_to_matrix(a.deg * (2.0 * u[9:12] - 1.0)).astype(np.float64) @ R
        t0 = pos + a.offset * d / np.sqrt((d * d).sum())
        truth.append((pos, R))
        multi.append((p * a.views, 0, (1 << a.views) - 1, R0, t0, 1.0))
        for k in range(a.views):
            ca, sa = np.cos(np.radians(yaws[k])), np.sin(np.radians(yaws[k]))
            Rc = np.array([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]])
            rig_R.append(Rc)
            rig_t.append(-(700.0 + 500.0 * u[12 + k]) * Rc[:, 2])
    V, uu = fit.views_from_rig(np.array(rig_R), np.array(rig_t))
    for p, (pos, R) in enumerate(truth):
        for k in range(a.views):
            c = p * a.views + k
            Vc, uc = V[c].astype(np.float64), uu[c].astype(np.float64)
            items += [(c, 0, Vc @ R, Vc @ pos + uc, 1.0, True), (c, 1, Vc, Vc @ pos + uc, 1.0, False)]
            single.append((c, 0, Vc @ multi[p][3], Vc @ multi[p][4] + uc, 1.0, False))
    m_inst = np.zeros(a.persons, _lib.VIEW_INSTANCE_DTYPE)
    for i, (first, model, views, R0, t0, scale) in enumerate(multi):
        m_inst[i] = (first, model, views, R0.astype(np.float32).reshape(9), t0.astype(np.float32), scale, 0)
    s_inst = render.instances(single)

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

    def geo(Ra, Rb):
        return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))))

    with render.Mesh(verts, tris) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd, fit.Model.from_mesh(verts, tris) as model, fit.Fitter() as ft, \
            Cameras(np.tile(K.reshape(1, 9), (n, 1))) as cams, fit.Views(cams, V, uu) as views:
        frames, _ = rd.render([head, torso], render.instances(items), n, w, h, cams, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        torch.cuda.synchronize()
        calls = {"views": lambda: ft.fit_views(frames, [model], m_inst, views, device_out=True),
                 "cameras": lambda: ft.fit(frames, [model], s_inst, cams, device_out=True)}
        meds = {"views": [], "cameras": []}
        for _ in range(a.runs):                                       # alternating, run after run
            for name in ("cameras", "views"):
                meds[name].append(run(calls[name]))
        m_out, m_rec = (x.cpu().numpy() for x in calls["views"]())
        s_out, s_rec = (x.cpu().numpy() for x in calls["cameras"]())
        torch.cuda.synchronize()
    m_out, m_rec = m_out.view(_lib.VIEW_INSTANCE_DTYPE), m_rec.view(_lib.VIEW_FIT_RECORD_DTYPE)
    s_out, s_rec = s_out.view(_lib.RENDER_INSTANCE_DTYPE), s_rec.view(_lib.FIT_RECORD_DTYPE)
    m_err = [(np.linalg.norm(m_out["t"][p] - pos), geo(m_out["R"][p].reshape(3, 3).astype(np.float64), R)) for p, (pos, R) in enumerate(truth)]
    s_err = []
    for p, (pos, R) in enumerate(truth):
        for k in range(a.views):
            c = p * a.views + k
            Vc, uc = V[c].astype(np.float64), uu[c].astype(np.float64)
            s_err.append((np.linalg.norm(s_out["t"][c] - (Vc @ pos + uc)), geo(s_out["R"][c].reshape(3, 3).astype(np.float64), Vc @ R)))

    def stat(v):
        return {"ms": float(np.median(v)), "min_run": min(v), "max_run": max(v)}

    print(json.dumps({"persons": a.persons, "views": a.views, "frames": n, "size": a.size, "points": len(verts),
                      "fit_views": stat(meds["views"]), "fit_cameras": stat(meds["cameras"]),
                      "views_over_cameras": float(np.median(meds["views"]) / np.median(meds["cameras"])),
                      "views_ok": int((m_rec["status"] == 0).sum()), "cameras_ok": int((s_rec["status"] == 0).sum()),
                      "views_err_mm_deg": [float(np.mean([e[0] for e in m_err])), float(np.mean([e[1] for e in m_err]))],
                      "cameras_err_mm_deg": [float(np.mean([e[0] for e in s_err])), float(np.mean([e[1] for e in s_err]))]}))


if __name__ == "__main__":
    main()
