"""Time the rig fit tracker's core device step on carried persons against the one-shot multi-view fit
with the default schedule (section 21) in the same process: `--rigs` rigs of `--views` cameras on an arc of +-35 degrees, one
head (`synth.head_mesh(--subdiv)` and a torso box) per rig at a seeded world pose, rendered twice -- the second time moved by
`--move` mm and `--turn` degrees of yaw -- into device-resident frames of `--size`.  The tracker is primed with one detected
step; then every timed step gets the other frame set, so each carried start lies one movement away from the head.
dh_fit_depth_views_device fits the same persons in the same frames from starts `--offset` mm and `--deg` degrees off with
the default schedule (20 coarse and full steps).  The two calls alternate, run after run.  Prints one JSON line: ms per call
measured with device events around each of `--steps` calls (after `--warmup`), as the median over the calls of each of `--runs`
repeats and the spread of those medians, for both; the statuses and mean step counts of the last carried step and its mean
errors against the rendered truth."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", type=int, default=64)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--offset", type=float, default=60.0)
    ap.add_argument("--deg", type=float, default=15.0)
    ap.add_argument("--move", type=float, default=5.0)
    ap.add_argument("--turn", type=float, default=2.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import _lib, fit, render, synth, tracking
    w, h = (int(v) for v in a.size.split("x"))
    n = a.rigs * a.views
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    yaws = np.linspace(-35.0, 35.0, a.views) if a.views > 1 else np.zeros(1)
    BIN = 3.14159 / 60.0
    rig_R, rig_t, truth, starts = [], [], ([], []), []
    for g in range(a.rigs):
        u = synth.SplitMix(53000 + g).uniform(15 + a.views)
        pos = 60.0 * (2.0 * u[:3] - 1.0)
        R = render.euler_to_matrix(np.array([30.0, 15.0, 10.0]) * (2.0 * u[3:6] - 1.0)).astype(np.float64)
        d, m = 2.0 * u[6:9] - 1.0, 2.0 * u[12:15] - 1.0
        d, m = d / np.sqrt((d * d).sum()), m / np.sqrt((m * m).sum())
        truth[0].append((pos, R))
        truth[1].append((pos + a.move * m, render.euler_to_matrix((0.0, a.turn, 0.0)).astype(np.float64) @ R))
        starts.append((render.euler_to_matrix(a.deg * (2.0 * u[9:12] - 1.0)).astype(np.float64), a.offset * d))
        for k in range(a.views):
            ca, sa = np.cos(np.radians(yaws[k])), np.sin(np.radians(yaws[k]))
            Rc = np.array([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]])
            rig_R.append(Rc)
            rig_t.append(-(700.0 + 500.0 * u[15 + k]) * Rc[:, 2])
    rig_R, rig_t = np.array(rig_R), np.array(rig_t)
    V, uu = fit.views_from_rig(rig_R, rig_t)
    rig_begin = np.arange(a.rigs + 1) * a.views
    items, m_inst, inputs = [[], []], [], []
    for s in (0, 1):
        inst = np.zeros(a.rigs, _lib.VIEW_INSTANCE_DTYPE)
        n_heads, heads = np.zeros(n, np.uint32), np.zeros((n, 1), _lib.HEAD_DTYPE)
        n_persons, persons = np.ones(a.rigs, np.uint32), np.zeros((a.rigs, _lib.RIG_MAX_PERSONS), _lib.RIG_PERSON_DTYPE)
        for g, (pos, R) in enumerate(truth[s]):
            c0 = g * a.views
            for k in range(a.views):
                Vc, uc = V[c0 + k].astype(np.float64), uu[c0 + k].astype(np.float64)
                items[s] += [(c0 + k, 0, Vc @ R, Vc @ pos + uc, 1.0, True), (c0 + k, 1, Vc, Vc @ pos + uc, 1.0, False)]
            dR, dt = starts[g]
            inst[g] = (c0, 0, (1 << a.views) - 1, (dR @ R).astype(np.float32).reshape(9), (pos + dt).astype(np.float32), 1.0, 0)
            p = persons[g, 0]
            p["views"], p["n_views"], p["world"], p["id"], p["best_cam"] = (1 << a.views) - 1, a.views, np.round(pos + dt), g + 1, c0
            heads[c0, 0]["pose"]["rotation"] = np.round(np.radians(fit.matrix_to_euler(V[c0].astype(np.float64) @ R)) / BIN) * BIN
            n_heads[c0] = 1
        m_inst.append(inst)
        inputs.append((n_heads, heads, n_persons, persons))

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()

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

    REC = _lib.RIG_FIT_RECORD_DTYPE
    with render.Mesh(verts, tris) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd, fit.Model.from_mesh(verts, tris) as model, fit.Fitter() as ft, \
            tracking.Cameras(np.tile(K.reshape(1, 9), (n, 1))) as cams, fit.Views(cams, V, uu) as views, \
            tracking.Rig(cams, rig_R.astype(np.float32), rig_t.astype(np.float32), rig_begin) as rig, \
            fit.RigFitTracker(rig, views, model, w, h) as tr:
        frames = [rd.render([head, torso], render.instances(items[s]), n, w, h, cams, noise=2, holes=0.02, seed=1 + s, device_out=True,
                            masks=False)[0] for s in (0, 1)]
        d_in = [[dev(x) for x in inputs[s]] for s in (0, 1)]
        d_rec = torch.zeros(a.rigs * _lib.RIG_MAX_TRACKS * REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        turn = {"track": 0, "views": 0}

        def track():
            s = turn["track"] = 1 - turn["track"]
            tr.step_device(frames[s].data_ptr(), *(x.data_ptr() for x in d_in[s]), d_rec.data_ptr(), max_heads=1)

        def one_shot():
            s = turn["views"] = 1 - turn["views"]
            return ft.fit_views(frames[s], [model], m_inst[s], views, device_out=True)

        tr.step_device(frames[0].data_ptr(), *(x.data_ptr() for x in d_in[0]), d_rec.data_ptr(), max_heads=1)    # prime: detected
        torch.cuda.synchronize()
        primed = d_rec.cpu().numpy().view(REC).reshape(a.rigs, -1)[:, 0]
        meds = {"track": [], "views": []}
        for _ in range(a.runs):                                       # alternating, run after run
            for name, call in (("views", one_shot), ("track", track)):
                meds[name].append(run(call))
        torch.cuda.synchronize()
        last = d_rec.cpu().numpy().view(REC).reshape(a.rigs, -1)[:, 0]
        s = turn["track"]
    err = [(np.linalg.norm(last["instance"]["t"][g] - pos), geo(last["instance"]["R"][g].reshape(3, 3).astype(np.float64), R))
           for g, (pos, R) in enumerate(truth[s])]

    def stat(v):
        return {"ms": float(np.median(v)), "min_run": min(v), "max_run": max(v)}

    print(json.dumps({"rigs": a.rigs, "views": a.views, "frames": n, "size": a.size, "points": len(verts),
                      "track_step": stat(meds["track"]), "fit_views": stat(meds["views"]),
                      "track_over_views": float(np.median(meds["track"]) / np.median(meds["views"])),
                      "primed_fitted": int((primed["status"] == fit.FIT_TRACK_FITTED).sum()),
                      "carried": int((last["status"] == fit.FIT_TRACK_CARRIED).sum()),
                      "carried_steps_mean": float(last["fit"]["steps"].mean()), "primed_steps_mean": float(primed["fit"]["steps"].mean()),
                      "carried_err_mm_deg": [float(np.mean([e[0] for e in err])), float(np.mean([e[1] for e in err]))]}))


if __name__ == "__main__":
    main()
