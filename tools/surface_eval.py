"""Time one surface step beside the shape step and the fit of the same batch, in one process:
`--subjects` subjects of `--frames` frames of `--size` each, every subject the generic head (`synth.head_mesh(--subdiv)`) with
two seeded bumps along its normals that `synth.head_basis` cannot express, one instance per frame started `--offset` mm and up to
`--deg` degrees per axis from the truth.
  the step      dh_fit_surface_subjects_device over all instances (device events, `--steps` calls after `--warmup`, `--runs` runs),
                and the same call with 0 sweeps, and with no instances (clear, solve, points and normals alone): the differences
                are the sweeps' and the accumulation's share;
  yardsticks    dh_fit_shape_subjects_device and dh_fit_depth_device on the same batch, timed the same way in the same process.
Then fit.refine_subjects for `--rounds` rounds from zero offsets: the fit's rms over all instances in the first and the last round.
Prints one JSON line of medians and their spread."""
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
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--offset", type=float, default=15.0)
    ap.add_argument("--deg", type=float, default=6.0)
    ap.add_argument("--max-offset", type=float, default=16.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import fit, render, synth, training
    from depthhead_amd._lib import FIT_RECORD_DTYPE
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    nrm = fit.vertex_normals(verts, tris)
    fields = synth.head_basis(verts)
    S, F = a.subjects, a.frames
    n = S * F
    face = np.flatnonzero(nrm[:, 2] < -0.5)
    heads = []
    for s in range(S):
        u = synth.SplitMix(4000 + s).uniform(2)
        disp = np.zeros(len(verts))
        for centre, height in ((face[int(u[0] * len(face))], 8.5), (face[int(u[1] * len(face))], -6.0)):
            d2 = ((verts.astype(np.float64) - verts[centre]) ** 2).sum(axis=1)
            disp += height * np.exp(-d2 / (2.0 * 22.0 * 22.0))
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
        frames = d_frames.cpu().view(torch.int16).numpy().view(np.uint16).reshape(n, h, w).copy()
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
        d_who = torch.from_numpy(who.view(np.int32)).cuda()
        seeded = starts.copy()
        seeded["mesh"] = who
        d_inst, d_frec = ft.fit(d_frames, st.models, seeded, K, device_out=True)
        torch.cuda.synchronize()
        none = d_inst[:0]
        zero = np.zeros(len(verts))
        no_sweeps = fit.surface_params(iterations=0)
        step, step0, tail, shape, fit_ms = [], [], [], [], []
        for _ in range(a.runs):
            step.append(events(lambda: ft.surface_step_subjects(d_frames, st, d_inst, K, subjects=d_who, fit_records=d_frec, device_out=True), a.steps, a.warmup))
            step0.append(events(lambda: ft.surface_step_subjects(d_frames, st, d_inst, K, subjects=d_who, fit_records=d_frec, params=no_sweeps, device_out=True),
                                a.steps, a.warmup))
            tail.append(events(lambda: ft.surface_step_subjects(d_frames, st, none, K, device_out=True), a.steps, a.warmup))
            shape.append(events(lambda: ft.shape_step_subjects(d_frames, st, d_inst, K, subjects=d_who, fit_records=d_frec, device_out=True), a.steps, a.warmup))
            fit_ms.append(events(lambda: ft.fit(d_frames, st.models, seeded, K, device_out=True), a.steps, a.warmup))
        # the quality of the alternation, from zero offsets
        for s in range(S):
            st.set_offsets(s, zero)

        def rms(records):
            ok = records["status"] == fit.FIT_OK
            return float(np.sqrt(records["sum_r2_fixed"][ok].sum() / 1048576.0 / records["points"][ok].sum()))

        _, first = ft.fit(frames, st.models, seeded, K)
        _, _, (last, urec) = fit.refine_subjects(ft, frames, K, st, starts, who, rounds=a.rounds)
        assert first.dtype == FIT_RECORD_DTYPE
    out = {"subjects": S, "frames_per_subject": F, "instances": n, "size": a.size, "points": len(verts), "runs": a.runs, "steps": a.steps,
           "surface_step_ms": spread(step), "surface_step_no_sweeps_ms": spread(step0), "surface_step_no_instances_ms": spread(tail),
           "shape_step_subjects_ms": spread(shape), "fit_ms": spread(fit_ms),
           "step_over_shape_step": float(np.median(step) / np.median(shape)), "step_over_fit": float(np.median(step) / np.median(fit_ms)),
           "rounds": a.rounds, "fit_rms_first_round_mm": rms(first), "fit_rms_last_round_mm": rms(last),
           "observed_mean": float(urec["observed"].mean()), "max_abs_mm": float(urec["max_abs"].max()), "clamped": int(urec["clamped"].sum()),
           "statuses_ok": bool((urec["status"] == fit.SURFACE_OK).all())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
