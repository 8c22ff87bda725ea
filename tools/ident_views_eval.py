"""Time one multi-view identification beside existing code doing the same work, in one process: `--rigs`
moments of a rig of `--views` cameras on an arc, `--size` each, every moment showing one of `--subjects` subjects -- the generic head
(`synth.head_mesh(--subdiv)`) with two seeded bumps along its normals, enrolled in a surface set by its true offsets -- at a seeded
world pose; one instance per moment, fitted over all its views with its own subject's model from a start `--offset` mm and up to
`--deg` degrees per axis off the truth.
  the call      dh_fit_identify_subjects_views_device over all instances (n_sets = --rigs, instance i in set i) and all subjects as
                candidates (device events, `--steps` calls after `--warmup`, `--runs` runs); the same with iterations = 0 (one pass
                a pair); and with nobody enrolled, where every pair leaves at once: both launches and the decide kernel;
  yardstick     dh_fit_depth_views_device over the same (instance, model) pairs -- instances x subjects of them, each naming its
                subject's model of the set, coarse_iterations = 0 and the call's iterations and gate, on a view table that repeats
                the rig once per moment so that one call reaches every moment's frames -- which is how a caller had to score a
                gallery over a rig before, short of the decision; and dh_fit_depth_views_device of the instances alone.
Prints one JSON line of medians and their spread, and how many instances were given their own subject."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=64)
    ap.add_argument("--rigs", type=int, default=64)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--offset", type=float, default=15.0)
    ap.add_argument("--deg", type=float, default=6.0)
    ap.add_argument("--half-arc", type=float, default=35.0)
    ap.add_argument("--distance", type=float, default=900.0)
    ap.add_argument("--max-offset", type=float, default=16.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import fit, render, synth, tracking
    from depthhead_amd._lib import IDENT_RECORD_DTYPE, VIEW_INSTANCE_DTYPE
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    nrm = fit.vertex_normals(verts, tris)
    fields = synth.head_basis(verts)
    S, M, C = a.subjects, a.rigs, a.views
    face = np.flatnonzero(nrm[:, 2] < -0.5)
    heads, bumps = [], []
    for s in range(S):
        u = synth.SplitMix(4000 + s).uniform(2)
        disp = np.zeros(len(verts))
        for centre, height in ((face[int(u[0] * len(face))], 8.5), (face[int(u[1] * len(face))], -6.0)):
            d2 = ((verts.astype(np.float64) - verts[centre]) ** 2).sum(axis=1)
            disp += height * np.exp(-d2 / (2.0 * 22.0 * 22.0))
        bumps.append(disp)
        heads.append(render.Mesh((verts.astype(np.float64) + disp[:, None] * nrm).astype(np.float32), tris))
    # the rig: cameras on an arc about the world's origin, each looking at it (camera to world, then the fit's direction)
    rig_R, rig_t = [], []
    for yaw in (np.linspace(-a.half_arc, a.half_arc, C) if C > 1 else [0.0]):
        ca, sa = np.cos(np.radians(yaw)), np.sin(np.radians(yaw))
        Rc = np.array([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]])
        rig_R.append(Rc)
        rig_t.append(-a.distance * Rc[:, 2])
    V, uu = fit.views_from_rig(np.array(rig_R), np.array(rig_t))
    who = (np.arange(M) % S).astype(np.uint32)
    items = []
    starts = np.zeros(M, VIEW_INSTANCE_DTYPE)
    for i in range(M):
        r = synth.SplitMix(52000 + i).uniform(12)
        pos = 60.0 * (2.0 * r[:3] - 1.0)
        R = render.euler_to_matrix(np.array([30.0, 15.0, 10.0]) * (2.0 * r[3:6] - 1.0)).astype(np.float64)
        for c in range(C):
            Vc, uc = V[c].astype(np.float64), uu[c].astype(np.float64)
            tc = Vc @ pos + uc
            items.append((i * C + c, int(who[i]), Vc @ R, tc, 1.0, True))
            items.append((i * C + c, S, Vc, tc, 1.0, False))
        d = 2.0 * r[6:9] - 1.0
        R0 = render.euler_to_matrix(a.deg * (2.0 * r[9:12] - 1.0)).astype(np.float64) @ R
        starts[i] = (i * C, who[i], (1 << C) - 1, R0.astype(np.float32).reshape(9), (pos + a.offset * d / np.sqrt((d * d).sum())).astype(np.float32), 1.0, 0)
    torso = render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0)))
    with render.Renderer() as rd:
        d_frames, _ = rd.render(heads + [torso], render.instances(items), M * C, w, h, K, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        torch.cuda.synchronize()
    for m in heads + [torso]:
        m.close()
    d_sets_of_frames = d_frames.reshape(M, C, h, w)

    def events(call, steps, warmup):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    Ks = np.ascontiguousarray(np.broadcast_to(K, (C, 3, 3)))
    with fit.Fitter() as ft, fit.ShapeBasis(fields) as basis, fit.Subjects(verts, tris, basis, S, max_offset=a.max_offset) as st, \
            tracking.Cameras(Ks) as cams, fit.Views(cams, V, uu) as views, tracking.Cameras(np.tile(Ks, (M, 1, 1))) as all_cams, \
            fit.Views(all_cams, np.tile(V, (M, 1, 1)), np.tile(uu, (M, 1))) as all_views:
        for s in range(S):
            st.set_offsets(s, bumps[s])
        d_inst, d_frec = ft.fit_views(d_frames, st.models, starts, all_views, device_out=True)
        torch.cuda.synchronize()
        fitted = d_inst.cpu().numpy().view(VIEW_INSTANCE_DTYPE)
        pairs = np.repeat(fitted, S)                                                # pair (i, s) at i * S + s, as the call orders them
        pairs["model"] = np.tile(np.arange(S, dtype=np.uint32), M)
        in_sets = fitted.copy()                                                     # the same instances as the identify call names them:
        in_sets["first_cam"] = 0                                                    # camera 0 of set i
        d_in_sets = torch.from_numpy(in_sets.view(np.uint8).reshape(-1).copy()).cuda()
        d_sets = torch.arange(M, dtype=torch.int32, device="cuda")
        prm = fit.ident_views_params()
        pair_prm = fit.fit_params(coarse_iterations=0, iterations=prm.iterations, gate=(prm.gate, prm.gate), lam=prm.lam, min_points=prm.min_points)
        one_pass = fit.ident_views_params(iterations=0)
        pair_pass = fit.fit_params(coarse_iterations=0, iterations=0, gate=(prm.gate, prm.gate), min_points=prm.min_points)
        nobody = torch.zeros(S, dtype=torch.uint8, device="cuda")

        def identify(**kw):
            return ft.identify_subjects_views(d_sets_of_frames, views, st, d_in_sets, sets=d_sets, fit_records=d_frec, device_out=True, **kw)

        ident, ident0, empty, pair_fit, pair_fit0, fit_ms = [], [], [], [], [], []
        for _ in range(a.runs):
            ident.append(events(lambda: identify(), a.steps, a.warmup))
            pair_fit.append(events(lambda: ft.fit_views(d_frames, st.models, pairs, all_views, params=pair_prm, device_out=True), a.steps, a.warmup))
            ident0.append(events(lambda: identify(params=one_pass), a.steps, a.warmup))
            pair_fit0.append(events(lambda: ft.fit_views(d_frames, st.models, pairs, all_views, params=pair_pass, device_out=True), a.steps, a.warmup))
            empty.append(events(lambda: identify(enrolled=nobody), a.steps, a.warmup))
            fit_ms.append(events(lambda: ft.fit_views(d_frames, st.models, starts, all_views, device_out=True), a.steps, a.warmup))
        d_sub, d_rec, _ = identify()
        torch.cuda.synchronize()
        sub, rec = d_sub.cpu().numpy().view(np.uint32), d_rec.cpu().numpy().view(IDENT_RECORD_DTYPE)
    out = {"subjects": S, "rigs": M, "views": C, "instances": M, "pairs": M * S, "size": a.size, "points": len(verts), "runs": a.runs, "steps": a.steps,
           "identify_ms": spread(ident), "fit_of_the_pairs_ms": spread(pair_fit), "identify_over_fit_of_the_pairs": float(np.median(ident) / np.median(pair_fit)),
           "identify_one_pass_ms": spread(ident0), "fit_of_the_pairs_one_pass_ms": spread(pair_fit0), "identify_nobody_enrolled_ms": spread(empty),
           "fit_of_the_instances_ms": spread(fit_ms), "right": int((sub == who).sum()), "best_right": int((rec["best"] == who).sum()),
           "statuses": {str(k): int((rec["status"] == k).sum()) for k in range(5)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
