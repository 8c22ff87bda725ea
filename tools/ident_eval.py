"""Time one identification beside existing code doing the same work, in one process: `--subjects` subjects
of `--frames` frames of `--size` each, every subject the generic head (`synth.head_mesh(--subdiv)`) with two seeded bumps along its
normals, enrolled in a surface set by its true offsets; one instance per frame, fitted with its own subject's model from a start
`--offset` mm and up to `--deg` degrees per axis off the truth.
  the call      dh_fit_identify_subjects_device over all instances and all subjects as candidates (device events, `--steps` calls
                after `--warmup`, `--runs` runs); the same with iterations = 0 (one pass a pair); and with nobody enrolled, where
                every pair leaves at once: both launches and the decide kernel, an upper bound of the decide kernel alone;
  yardstick     dh_fit_depth_device over the same (instance, model) pairs -- instances x subjects of them, each naming its
                subject's model of the set, coarse_iterations = 0 and the call's iterations and gate -- which is how a caller
                had to score a gallery before, short of the decision; and dh_fit_depth_device of the instances alone.
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
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--offset", type=float, default=15.0)
    ap.add_argument("--deg", type=float, default=6.0)
    ap.add_argument("--max-offset", type=float, default=16.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import fit, render, synth, training
    from depthhead_amd._lib import IDENT_RECORD_DTYPE, RENDER_INSTANCE_DTYPE
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    nrm = fit.vertex_normals(verts, tris)
    fields = synth.head_basis(verts)
    S, F = a.subjects, a.frames
    n = S * F
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
    items, start = [], []
    for f in range(n):
        pos, rot = training.rendered_pose(w, h, training.RENDER_SEED_BASE + f)
        R = render.euler_to_matrix(rot)
        items.append((f, f // F, R, pos, 1.0, True))
        items.append((f, S, np.eye(3), pos, 1.0, False))
        u = synth.SplitMix(31337 + f).uniform(6)
        d = 2.0 * u[:3] - 1.0
        R0 = render.euler_to_matrix(a.deg * (2.0 * u[3:] - 1.0)).astype(np.float64) @ R.astype(np.float64)
        start.append((f, 0, R0, pos + a.offset * d / np.sqrt((d * d).sum()), 1.0, False))
    starts = render.instances(start)
    who = (np.arange(n) // F).astype(np.uint32)
    torso = render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0)))
    with render.Renderer() as rd:
        d_frames, _ = rd.render(heads + [torso], render.instances(items), n, w, h, K, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        torch.cuda.synchronize()
    for m in heads + [torso]:
        m.close()

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

    with fit.Fitter() as ft, fit.ShapeBasis(fields) as basis, fit.Subjects(verts, tris, basis, S, max_offset=a.max_offset) as st:
        for s in range(S):
            st.set_offsets(s, bumps[s])
        seeded = starts.copy()
        seeded["mesh"] = who
        d_inst, d_frec = ft.fit(d_frames, st.models, seeded, K, device_out=True)
        torch.cuda.synchronize()
        fitted = d_inst.cpu().numpy().view(RENDER_INSTANCE_DTYPE)
        pairs = np.repeat(fitted, S)                                                # pair (i, s) at i * S + s, as the call orders them
        pairs["mesh"] = np.tile(np.arange(S, dtype=np.uint32), n)
        prm = fit.ident_params()
        pair_prm = fit.fit_params(coarse_iterations=0, iterations=prm.iterations, gate=(prm.gate, prm.gate), lam=prm.lam, min_points=prm.min_points)
        one_pass, pair_pass = fit.ident_params(iterations=0), fit.fit_params(coarse_iterations=0, iterations=0, gate=(prm.gate, prm.gate), min_points=prm.min_points)
        nobody = torch.zeros(S, dtype=torch.uint8, device="cuda")
        ident, ident0, empty, pair_fit, pair_fit0, fit_ms = [], [], [], [], [], []
        for _ in range(a.runs):
            ident.append(events(lambda: ft.identify_subjects(d_frames, st, d_inst, K, fit_records=d_frec, device_out=True), a.steps, a.warmup))
            pair_fit.append(events(lambda: ft.fit(d_frames, st.models, pairs, K, params=pair_prm, device_out=True), a.steps, a.warmup))
            ident0.append(events(lambda: ft.identify_subjects(d_frames, st, d_inst, K, fit_records=d_frec, params=one_pass, device_out=True), a.steps, a.warmup))
            pair_fit0.append(events(lambda: ft.fit(d_frames, st.models, pairs, K, params=pair_pass, device_out=True), a.steps, a.warmup))
            empty.append(events(lambda: ft.identify_subjects(d_frames, st, d_inst, K, enrolled=nobody, fit_records=d_frec, device_out=True), a.steps, a.warmup))
            fit_ms.append(events(lambda: ft.fit(d_frames, st.models, seeded, K, device_out=True), a.steps, a.warmup))
        d_sub, d_rec, _ = ft.identify_subjects(d_frames, st, d_inst, K, fit_records=d_frec, device_out=True)
        torch.cuda.synchronize()
        sub, rec = d_sub.cpu().numpy().view(np.uint32), d_rec.cpu().numpy().view(IDENT_RECORD_DTYPE)
    out = {"subjects": S, "frames_per_subject": F, "instances": n, "pairs": n * S, "size": a.size, "points": len(verts), "runs": a.runs, "steps": a.steps,
           "identify_ms": spread(ident), "fit_of_the_pairs_ms": spread(pair_fit), "identify_over_fit_of_the_pairs": float(np.median(ident) / np.median(pair_fit)),
           "identify_one_pass_ms": spread(ident0), "fit_of_the_pairs_one_pass_ms": spread(pair_fit0), "identify_nobody_enrolled_ms": spread(empty),
           "fit_of_the_instances_ms": spread(fit_ms), "right": int((sub == who).sum()), "best_right": int((rec["best"] == who).sum()),
           "statuses": {str(k): int((rec["status"] == k).sum()) for k in range(5)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
