"""Time the adaptation of many subjects at once against the way it was done before, in one process:
`--subjects` subjects of `--frames` frames of `--size` each, every subject the generic head (`synth.head_mesh(--subdiv)`)
stretched by its own seeded amount within +-0.1 per axis, one instance per frame started `--offset` mm and up to `--deg` degrees
per axis from the truth, the first `--fields` fields of `synth.head_basis`, `--rounds` rounds.
  device path   fit.adapt_subjects over one fit.Subjects set: wall clock around the call (the upload of the frames and the one read
                at the end included), and device events around its rounds alone with the frames already on the device;
  yardstick     fit.adapt called once per subject on that subject's frames: wall clock.
The two alternate, `--runs` times each; medians and their spread.  Then one dh_fit_subjects_update_device alone against the shape
step over the set and dh_fit_shape_device on the same batch (device events, `--steps` calls after `--warmup`, per run).  Prints one
JSON line, with whether both paths reached the same coefficients."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--fields", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--offset", type=float, default=15.0)
    ap.add_argument("--deg", type=float, default=6.0)
    a = ap.parse_args()
    import torch
    from depthhead_amd import fit, render, synth, training
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    full = synth.head_basis(verts)
    fields = full[:a.fields]
    S, F = a.subjects, a.frames
    n = S * F
    truth = 0.2 * synth.SplitMix(2025).uniform(S * 3).reshape(S, 3) - 0.1
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

    heads = [render.Mesh(fit.deform(verts, full, list(truth[s]) + [0.0]), tris) for s in range(S)]
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

    with fit.Fitter() as ft, fit.ShapeBasis(fields) as basis, fit.Subjects(verts, tris, basis, S) as st, fit.Model.from_mesh(verts, tris) as generic:
        zeros = np.zeros((S, a.fields))

        def device_path():
            st.set_coeffs(zeros)
            t0 = time.perf_counter()
            state, inst, _ = fit.adapt_subjects(ft, frames, K, st, starts, who, rounds=a.rounds)
            return (time.perf_counter() - t0) * 1e3, state["coeffs"][:, :a.fields].copy()

        d_who = torch.from_numpy(who.view(np.int32)).cuda()
        seeded = starts.copy()
        seeded["mesh"] = who

        def rounds_alone():
            """The rounds of fit.adapt_subjects with the frames already on the device: what the device does, by its own clock."""
            st.set_coeffs(zeros)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d_inst = None
            for _ in range(a.rounds):
                d_inst, d_frec = ft.fit(d_frames, st.models, seeded, K, device_out=True, carried=d_inst)
                d_srec = ft.shape_step_subjects(d_frames, st, d_inst, K, subjects=d_who, fit_records=d_frec, device_out=True)
                st.update(d_srec, device=True)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def local(starts_of_subject):
            out = starts_of_subject.copy()
            out["frame"] -= out["frame"][0]
            return out

        def yardstick():
            """fit.adapt per subject, on that subject's frames numbered from 0."""
            t0 = time.perf_counter()
            out = [fit.adapt(ft, frames[s * F:(s + 1) * F], K, verts, tris, fields, local(starts[s * F:(s + 1) * F]), rounds=a.rounds)[0] for s in range(S)]
            return (time.perf_counter() - t0) * 1e3, np.array(out)

        device_path(), rounds_alone(), yardstick()                       # warm every shape both paths use
        wall_dev, ev_dev, wall_old = [], [], []
        for _ in range(a.runs):
            ms, c_dev = device_path()
            wall_dev.append(ms)
            ev_dev.append(rounds_alone())
            ms, c_old = yardstick()
            wall_old.append(ms)
        # one update alone, beside the shape steps of the same batch
        d_inst, d_frec = ft.fit(d_frames, st.models, seeded, K, device_out=True)
        d_srec = ft.shape_step_subjects(d_frames, st, d_inst, K, subjects=d_who, fit_records=d_frec, device_out=True)
        torch.cuda.synchronize()
        quiet = torch.zeros_like(d_srec)                                        # records of status OK and zero increments: nothing moves
        upd, step_set, step_one, fit_ms = [], [], [], []
        for _ in range(a.runs):
            upd.append(events(lambda: st.update(quiet, device=True), a.steps, a.warmup))
            step_set.append(events(lambda: ft.shape_step_subjects(d_frames, st, d_inst, K, subjects=d_who, fit_records=d_frec, device_out=True), a.steps, a.warmup))
            step_one.append(events(lambda: ft.shape_step(d_frames, generic, basis, d_inst, K, device_out=True), a.steps, a.warmup))
            fit_ms.append(events(lambda: ft.fit(d_frames, st.models, seeded, K, device_out=True), a.steps, a.warmup))
        state = st.state()
    out = {"subjects": S, "frames_per_subject": F, "size": a.size, "points": len(verts), "fields": a.fields, "rounds": a.rounds, "runs": a.runs,
           "adapt_subjects_wall_ms": spread(wall_dev), "adapt_subjects_rounds_device_ms": spread(ev_dev), "adapt_per_subject_wall_ms": spread(wall_old),
           "speedup_wall": float(np.median(wall_old) / np.median(wall_dev)),
           "same_coefficients": bool(c_dev.tobytes() == c_old.tobytes()), "max_abs_difference": float(np.abs(c_dev - c_old).max()),
           "max_abs_error_xyz": float(np.abs(c_dev[:, :3] - truth).max()) if a.fields >= 3 else None,
           "update_ms": spread(upd), "shape_step_subjects_ms": spread(step_set), "shape_step_one_model_ms": spread(step_one), "fit_ms": spread(fit_ms),
           "update_bytes": int(S * len(verts) * (12 + 12 * a.fields + 12 + 12 + 6 * 9 * 4)),
           "applied": state["applied"].tolist()[:4], "flags_any": bool(state["flags"].any())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
