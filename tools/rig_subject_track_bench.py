"""Time the rig subject fit tracker: `--rigs` rigs of `--cameras` cameras of `--size` on an arc, each rig
seeing one rendered head (`synth.head_mesh(--subdiv)`) and its torso box through all its cameras, a gallery of `--subjects`
subjects of that mesh (seeded coefficients of `synth.head_basis` within +-`--spread`: small, so that every subject's model still
fits the rendered generic head and a bound entry stays bound), device-resident frames and outputs, the core step from persons
faked as the truth plus `--offset` mm.  Each figure is the median (and spread) of `--runs` run medians over `--steps` calls after
`--warmup`, in ms per step of all rigs, measured with device events; pairs are timed alternately, call by call, so that both see
the same clocks:
  (a) a steady-state step with every entry bound (dh_rig_subject_fit_tracker_step_persons_device) against RigFitTracker's carried
      step (dh_rig_fit_tracker_step_persons_device);
  (b) a step in which every entry wants identification (a limit no head meets, retry 0, no try limit) against the existing path
      on the device: dh_rig_fit_tracker_step_persons_device, then dh_fit_identify_subjects_views_device over all slots;
  (c) the same with one slot in all wanting (the others bound by the caller) against the same path, the fit records of the other
      slots marked not-OK -- what a caller without the list would launch.
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


def arc(yaws_deg, dist):
    """Camera-to-world extrinsics of cameras on an arc about the world origin, each looking at it from `dist` mm."""
    R, t = [], []
    for a in yaws_deg:
        ca, sa = np.cos(np.radians(a)), np.sin(np.radians(a))
        Rc = np.array([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]])
        R.append(Rc)
        t.append(-dist * Rc[:, 2])
    return np.array(R), np.array(t)


def measure(a) -> dict:
    import torch
    from depthhead_amd import _lib, fit, render, synth, tracking
    ng, nc, S = a.rigs, a.cameras, a.subjects
    n, slots = ng * nc, ng * _lib.RIG_MAX_TRACKS
    w, h = (int(v) for v in a.size.split("x"))
    K = synth.default_intrinsic(w, h)
    verts, tris = synth.head_mesh(a.subdiv)
    basis = synth.head_basis(verts)
    Ra, ta = arc(np.linspace(-30.0, 30.0, nc) if nc > 1 else [0.0], a.distance)
    rig_R, rig_t = np.tile(Ra, (ng, 1, 1)).astype(np.float32), np.tile(ta, (ng, 1)).astype(np.float32)
    V, u = fit.views_from_rig(rig_R, rig_t)
    rig_begin = [g * nc for g in range(ng + 1)]
    items = []
    n_heads, heads = np.zeros(n, np.uint32), np.zeros((n, 1), _lib.HEAD_DTYPE)
    n_persons, persons = np.ones(ng, np.uint32), np.zeros((ng, _lib.RIG_MAX_PERSONS), _lib.RIG_PERSON_DTYPE)
    bin_ = 3.14159 / 60.0
    for g in range(ng):
        r = synth.SplitMix(515151 + g).uniform(6)
        pos = 50.0 * (2.0 * r[:3] - 1.0)
        R = render.euler_to_matrix(np.array([20.0, 10.0, 8.0]) * (2.0 * r[3:] - 1.0)).astype(np.float64)
        for c in range(g * nc, (g + 1) * nc):
            Vc, uc = V[c].astype(np.float64), u[c].astype(np.float64)
            items.append((c, 0, Vc @ R, Vc @ pos + uc, 1.0, True))
            items.append((c, 1, Vc, Vc @ pos + uc, 1.0, False))
        d = 2.0 * synth.SplitMix(31337 + g).uniform(3) - 1.0
        p, b = persons[g, 0], g * nc
        p["views"], p["n_views"], p["mass"], p["id"], p["best_cam"], p["best_head"] = (1 << nc) - 1, nc, 100 * nc, 1, b, 0
        p["world"] = np.round(pos + a.offset * d / np.sqrt((d * d).sum()))
        n_heads[b] = 1
        heads[b, 0]["pose"]["mid_point"] = np.round(V[b].astype(np.float64) @ p["world"].astype(np.float64) + u[b])
        heads[b, 0]["pose"]["rotation"] = np.round(np.radians(fit.matrix_to_euler(V[b].astype(np.float64) @ R)) / bin_) * bin_
        heads[b, 0]["support"]["windows"], heads[b, 0]["support"]["mass"], heads[b, 0]["support"]["total_mass"] = 10, 100, 1000
    coeffs = a.spread * (2.0 * synth.SplitMix(4242).uniform(S * len(basis)).reshape(S, len(basis)) - 1.0)
    prm = fit.rig_fit_track_params(max_jump=4096.0)
    never = fit.ident_views_params(max_rms=1e-6)                 # every identification ends DH_IDENT_FAR: nobody is ever bound by it
    every = fit.subject_track_params(retry=0, max_tries=0)
    dev = torch.device("cuda", 0)

    def dbuf(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def up(array):
        return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(dev)

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

    out = {"rigs": ng, "cameras": nc, "size": a.size, "points": len(verts), "subjects": S}
    REC, PLAIN = _lib.RIG_SUBJECT_RECORD_DTYPE, _lib.RIG_FIT_RECORD_DTYPE
    with render.Mesh(verts, tris) as head, render.Mesh(*synth.box_mesh((-142.0, 85.0, 50.0), (142.0, 700.0, 250.0))) as torso, \
            render.Renderer() as rd, fit.Model.from_mesh(verts, tris) as model, fit.Fitter() as ft, fit.ShapeBasis(basis) as sb, \
            fit.Subjects(verts, tris, sb, S) as gallery, tracking.Cameras(np.tile(K.reshape(1, 9), (n, 1))) as cams, \
            tracking.Rig(cams, rig_R, rig_t, rig_begin) as rig, fit.Views(cams, V, u) as views, \
            fit.RigFitTracker(rig, views, model, w, h, params=prm) as plain, \
            fit.RigSubjectFitTracker(rig, views, gallery, model, w, h, params=prm, ident_params=never, subject_params=every) as tr:
        gallery.set_coeffs(coeffs)
        frames, _ = rd.render([head, torso], render.instances(items), n, w, h, K, noise=2, holes=0.02, seed=1, device_out=True, masks=False)
        s = torch.cuda.current_stream(dev).cuda_stream
        d_nh, d_hd, d_np, d_pn = up(n_heads), up(heads), up(n_persons), up(persons)
        d_r, d_q = dbuf(slots * REC.itemsize), dbuf(slots * PLAIN.itemsize)
        out["score_workgroups"] = tr.info()[2]

        def records():
            torch.cuda.synchronize()
            r = d_r.cpu().numpy().view(REC)
            live = r[r["track"]["status"] != 0]
            return {"kinds": np.bincount(r["track"]["status"] & 0xFF, minlength=5).tolist(), "identified": int(r["identified"].sum()),
                    "bound": int((r["subject"] != 0xFFFFFFFF).sum()), "steps_mean": float(live["track"]["fit"]["steps"].mean()) if len(live) else 0.0}

        def step():
            tr.step_device(frames.data_ptr(), d_nh.data_ptr(), d_hd.data_ptr(), d_np.data_ptr(), d_pn.data_ptr(), d_r.data_ptr(), max_heads=1, stream=s)

        def plain_step():
            plain.step_device(frames.data_ptr(), d_nh.data_ptr(), d_hd.data_ptr(), d_np.data_ptr(), d_pn.data_ptr(), d_q.data_ptr(), max_heads=1, stream=s)

        # the existing path's identification: the plain tracker's instances and fit records, gathered once (the copy is not timed)
        plain_step(); plain_step()
        torch.cuda.synchronize()
        q = d_q.cpu().numpy().view(PLAIN)
        d_inst = up(q["instance"])
        frec_all = np.ascontiguousarray(q["fit"])
        frec_all["status"][(q["status"] & 0xFF) == 0] = 1        # an unused slot: DH_FIT_FEW_POINTS, it takes no part
        frec_one = frec_all.copy()
        frec_one["status"][1:] = 1                               # only slot 0 takes part
        d_frec_all, d_frec_one = up(frec_all), up(frec_one)
        d_subj, d_irec = dbuf(slots * 4), dbuf(slots * _lib.IDENT_RECORD_DTYPE.itemsize)
        lib, vp = _lib.load(), _lib.vp

        def identify(d_frec):
            # the C call with outputs allocated once, so that the host does between the launches what the tracker's step does
            _lib.check(lib.dh_fit_identify_subjects_views_device(ft._h, vp(frames.data_ptr()), C.c_uint32(1), w, h, views._h, gallery._h,
                                                                 vp(d_inst.data_ptr()), C.c_uint32(slots), None, None, C.c_uint32(S),
                                                                 vp(d_frec.data_ptr()), C.byref(never), vp(d_subj.data_ptr()),
                                                                 vp(d_irec.data_ptr()), None, None, C.c_void_p(s)))

        identify(d_frec_all)                                     # (the fitter's pair scratch grows here)
        torch.cuda.synchronize()

        def existing(d_frec):
            plain_step()
            identify(d_frec)

        # (b) every entry wants identification at every step
        step(); step()
        out["b_all_want"], out["b_existing"] = timed_pair(step, lambda: existing(d_frec_all))
        out["b_all_want"].update(records())
        # (c) one slot wants, the others are bound by the caller
        for g in range(1, ng):
            tr.bind(g, 1, g % S, stream=s)
        step()
        out["c_one_wants"], out["c_existing"] = timed_pair(step, lambda: existing(d_frec_one))
        out["c_one_wants"].update(records())
        # (a) every entry bound
        tr.bind(0, 1, 0, stream=s)
        step()
        out["a_all_bound"], out["a_rig_fit_tracker"] = timed_pair(step, plain_step)
        out["a_all_bound"].update(records())
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", type=int, default=64)
    ap.add_argument("--cameras", type=int, default=4)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--subjects", type=int, default=64)
    ap.add_argument("--distance", type=float, default=900.0)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--offset", type=float, default=60.0)
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
    for key in ("a_all_bound", "a_rig_fit_tracker", "b_all_want", "b_existing", "c_one_wants", "c_existing"):
        v = [o[key]["event_ms"] for o in outs]
        merged[key] = dict(outs[0][key], event_ms=float(np.median(v)), event_ms_processes=[min(v), max(v)])
    merged["processes"] = a.processes
    print(json.dumps(merged))


if __name__ == "__main__":
    main()
