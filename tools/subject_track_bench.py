"""Time the subject fit tracker: `--cameras` cameras of `--size`, each seeing a rendered head
(`synth.head_mesh(--subdiv)`) and its torso box, a gallery of `--subjects` subjects of that mesh (seeded coefficients of
`synth.head_basis` within +-`--spread`: small, so that every subject's model still fits the rendered generic head and a bound
camera stays bound), device-resident frames and outputs, the core step from poses faked as the truth plus `--offset` mm.  Each
figure is the median (and spread) of `--runs` run medians over `--steps` calls after `--warmup`, in ms per step of all cameras,
measured with device events; pairs are timed alternately, call by call, so that both see the same clocks:
  (a) a steady-state step with every camera bound (dh_subject_fit_tracker_step_poses_device) against FitTracker's carried step
      (dh_fit_tracker_step_poses_device);
  (b) a step in which every camera wants identification (a limit no head meets, retry 0, no try limit) against the existing
      path on the device: dh_fit_tracker_step_poses_device, then dh_fit_identify_subjects_cameras_device over all cameras;
  (c) the same with one camera in all wanting (the others bound by the caller) against the same path, the fit records of the
      other cameras marked not-OK -- what a caller without the list would launch.
With `--processes` > 1 the measurement runs in that many fresh child processes one after another and the medians of their
figures are reported with their spread.  One JSON line."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(a) -> dict:
    import torch
    from depthhead_amd import _lib, fit, render, synth, tracking, training
    n, S = a.cameras, a.subjects
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    basis = synth.head_basis(verts)
    items = []
    poses = np.zeros(n, _lib.POSE_DTYPE)
    support = np.zeros(n, _lib.SUPPORT_DTYPE)
    support["windows"], support["mass"], support["total_mass"] = 10, 100, 1000
    bin_ = 3.14159 / 60.0
    for f in range(n):
        pos, rot = training.rendered_pose(w, h, training.RENDER_SEED_BASE + f)
        items.append((f, 0, render.euler_to_matrix(rot), pos, 1.0, True))
        items.append((f, 1, np.eye(3), pos, 1.0, False))
        d = 2.0 * synth.SplitMix(31337 + f).uniform(3) - 1.0
        poses["mid_point"][f] = np.round(pos + a.offset * d / np.sqrt((d * d).sum()))
        poses["rotation"][f] = np.round(np.radians(rot.astype(np.float64)) / bin_) * bin_
    coeffs = a.spread * (2.0 * synth.SplitMix(4242).uniform(S * len(basis)).reshape(S, len(basis)) - 1.0)
    prm = fit.fit_track_params(conf=(0, 1), min_windows=0, max_jump=4096.0)
    never = fit.ident_params(max_rms=1e-6)                       # every identification ends DH_IDENT_FAR: nobody is ever bound by it
    every = fit.subject_track_params(retry=0, max_tries=0)
    dev = torch.device("cuda", 0)

    def dbuf(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def timed_pair(fa, fb):
        """fa and fb alternately, call by call: two dicts of the run medians' median and spread (device-event ms per call)."""
        runs = ([], [])
        for _ in range(a.runs):
            e = ([], [])
            for i in range(a.warmup + a.steps):
                for k, fn in enumerate((fa, fb)):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        e[k].append(e0.elapsed_time(e1))
            for k in (0, 1):
                runs[k].append(float(np.median(e[k])))
        return tuple({"event_ms": float(np.median(r)), "event_ms_runs": [min(r), max(r)]} for r in runs)

    out = {"cameras": n, "size": a.size, "points": len(verts), "subjects": S}
    with render.Mesh(verts, tris) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd, fit.Model.from_mesh(verts, tris) as model, fit.Fitter() as ft, fit.ShapeBasis(basis) as sb, \
            fit.Subjects(verts, tris, sb, S) as gallery, tracking.Cameras(np.tile(K.reshape(1, 9), (n, 1))) as cams, \
            fit.FitTracker(cams, model, w, h, params=prm) as plain, \
            fit.SubjectFitTracker(cams, gallery, model, w, h, params=prm, ident_params=never, subject_params=every) as tr:
        gallery.set_coeffs(coeffs)
        frames, _ = rd.render([head, torso], render.instances(items), n, w, h, K, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        s = torch.cuda.current_stream(dev).cuda_stream
        d_p = torch.from_numpy(poses.view(np.uint8).copy()).to(dev)
        d_s = torch.from_numpy(support.view(np.uint8).copy()).to(dev)
        d_r, d_q = dbuf(n * _lib.SUBJECT_TRACK_RECORD_DTYPE.itemsize), dbuf(n * _lib.FIT_TRACK_RECORD_DTYPE.itemsize)
        out["score_workgroups"] = tr.info()[2]

        def records():
            torch.cuda.synchronize()
            r = d_r.cpu().numpy().view(_lib.SUBJECT_TRACK_RECORD_DTYPE)
            return {"kinds": np.bincount(r["track"]["status"] & 0xFF, minlength=5).tolist(), "identified": int(r["identified"].sum()),
                    "bound": int((r["subject"] != 0xFFFFFFFF).sum()), "steps_mean": float(r["track"]["fit"]["steps"].mean())}

        def step():
            tr.step_device(frames.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_r.data_ptr(), stream=s)

        def plain_step():
            plain.step_device(frames.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_q.data_ptr(), stream=s)

        # the existing path's identification: the plain tracker's instances and fit records, gathered once (the copy is not timed)
        plain_step(); plain_step()
        torch.cuda.synchronize()
        q = d_q.cpu().numpy().view(_lib.FIT_TRACK_RECORD_DTYPE)
        d_inst = torch.from_numpy(np.ascontiguousarray(q["instance"]).view(np.uint8).reshape(-1).copy()).to(dev)
        frec_all = np.ascontiguousarray(q["fit"])
        frec_one = frec_all.copy()
        frec_one["status"][1:] = 1                               # DH_FIT_FEW_POINTS: only camera 0 takes part
        d_frec_all = torch.from_numpy(frec_all.view(np.uint8).reshape(-1).copy()).to(dev)
        d_frec_one = torch.from_numpy(frec_one.view(np.uint8).reshape(-1).copy()).to(dev)
        d_subj, d_irec = dbuf(n * 4), dbuf(n * _lib.IDENT_RECORD_DTYPE.itemsize)
        lib, vp = _lib.load(), _lib.vp

        def identify(d_frec):
            # the C call with outputs allocated once, so that the host does between the launches what the tracker's step does
            _lib.check(lib.dh_fit_identify_subjects_cameras_device(ft._h, vp(frames.data_ptr()), n, w, h, cams._h, gallery._h, vp(d_inst.data_ptr()),
                                                                   C.c_uint32(n), None, C.c_uint32(S), vp(d_frec.data_ptr()), C.byref(never),
                                                                   vp(d_subj.data_ptr()), vp(d_irec.data_ptr()), None, None, C.c_void_p(s)))

        identify(d_frec_all)                                     # (the fitter's pair scratch grows here)
        torch.cuda.synchronize()

        def existing(d_frec):
            plain_step()
            identify(d_frec)

        # (b) every camera wants identification at every step
        step(); step()
        out["b_all_want"], out["b_existing"] = timed_pair(step, lambda: existing(d_frec_all))
        out["b_all_want"].update(records())
        # (c) one camera wants, the others are bound by the caller
        for c in range(1, n):
            tr.bind(c, c % S, stream=s)
        step()
        out["c_one_wants"], out["c_existing"] = timed_pair(step, lambda: existing(d_frec_one))
        out["c_one_wants"].update(records())
        # (a) every camera bound
        tr.bind(0, 0, stream=s)
        step()
        out["a_all_bound"], out["a_fit_tracker"] = timed_pair(step, plain_step)
        out["a_all_bound"].update(records())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=256)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--subjects", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--offset", type=float, default=90.0)
    ap.add_argument("--spread", type=float, default=0.02)
    ap.add_argument("--processes", type=int, default=1)
    a = ap.parse_args()
    if a.processes <= 1:
        print(json.dumps(measure(a)))
        return
    argv = [v for i, v in enumerate(sys.argv[1:]) if v != "--processes" and (i == 0 or sys.argv[i] != "--processes")]
    outs = []
    for _ in range(a.processes):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], capture_output=True, text=True, check=True)
        outs.append(json.loads(res.stdout.strip().splitlines()[-1]))
    merged = dict(outs[0])
    for key in ("a_all_bound", "a_fit_tracker", "b_all_want", "b_existing", "c_one_wants", "c_existing"):
        v = [o[key]["event_ms"] for o in outs]
        merged[key] = dict(outs[0][key], event_ms=float(np.median(v)), event_ms_processes=[min(v), max(v)])
    merged["processes"] = a.processes
    print(json.dumps(merged))


if __name__ == "__main__":
    main()
