"""Scenes shared by the calibration tests (test_calib_ref.py on the CPU, test_gpu_calibrate.py on the GPU): section 21's arc
cameras (view_fit_scenes.arc: -35, 0 and +35 degrees about the world origin) see ONE head (head_mesh(2)) with its torso box
at several SETS, the head spread over the working volume -- up to +-200 / 120 / 150 mm from the origin, yaw +-30, pitch +-15,
roll +-10 degrees -- rendered by the renderer's restatement with the sensor model (noise 2, holes 0.02 unless told otherwise).
The middle camera is the gauge; `perturbed` moves the two outer ones off by a seeded rotation and a seeded 3-d offset.  Every
array is computed once and handed out read-only."""
import functools

import numpy as np

import fit_scenes as fs
import render_ref as rr
import view_fit_scenes as vs
from depthhead_amd import fit, render, synth

YAWS = (-35.0, 0.0, 35.0)
MIDDLE = 1                              # the camera at yaw 0: held
HOLD = (0, 1, 0)
SPREAD = (200.0, 120.0, 150.0)          # mm: the head's positions lie within this of the origin, per axis


@functools.lru_cache(maxsize=None)
def rig(seed, n_sets=6, w=160, h=120, noise=2, holes=0.02, spread=SPREAD):
    """(frames [n_sets, 3, h, w] u16, Ks [3, 3, 3] f32, the TRUE V [3, 3, 3] f32 and u [3, 3] f32, true world positions [n_sets, 3]
    f64, true world R [n_sets, 3, 3] f64) of rig `seed`."""
    rng = synth.SplitMix(770000 + seed)
    dists = vs.truth(1000 * seed)[2]
    V, u = fit.views_from_rig(*vs.arc(YAWS, dists))
    K = synth.default_intrinsic(w, h)
    v, t, _ = fs.head()
    n = len(YAWS)
    items, pos, Rs = [], [], []
    for s in range(n_sets):
        uu = rng.uniform(6)
        p = np.array(spread) * (2.0 * uu[:3] - 1.0)
        R = render.euler_to_matrix(np.array([30.0, 15.0, 10.0]) * (2.0 * uu[3:] - 1.0)).astype(np.float64)
        items += [rr.instance(f, m, Rc, tc, head=hd) for f, m, Rc, tc, _, hd in vs.view_items(p, R, V, u, first=s * n)]
        pos.append(p)
        Rs.append(R)
    frames, _ = rr.render([(v, t), fs.torso()], items, n_sets * n, w, h, K, noise=noise, holes=holes, seed=seed)
    Ks = np.ascontiguousarray(np.broadcast_to(K, (n, 3, 3)))
    return vs._ro(frames.reshape(n_sets, n, h, w), Ks, V, u, np.array(pos), np.array(Rs))


@functools.lru_cache(maxsize=None)
def perturbed(seed, off_mm=20.0, off_deg=2.0):
    """(V [3, 3, 3] f32, u [3, 3] f32) of rig `seed` with the two outer cameras off: turned by up to off_deg degrees per axis
    and moved by off_mm in a seeded direction (V = C V_true, u = C u_true + d); the middle camera is true."""
    Vt, ut = rig(seed)[2:4]
    V, u = Vt.astype(np.float64), ut.astype(np.float64)
    rng = synth.SplitMix(880000 + seed)
    for c in (0, 2):
        uu = rng.uniform(6)
        C = render.euler_to_matrix(off_deg * (2.0 * uu[:3] - 1.0)).astype(np.float64)
        d = 2.0 * uu[3:] - 1.0
        d = off_mm * d / np.linalg.norm(d)
        V[c], u[c] = C @ V[c], C @ u[c] + d
    return vs._ro(V.astype(np.float32), u.astype(np.float32))


def true_instances(pos, Rs, views=0b111):
    """The true world poses as instance dicts (set s is instance s; first_cam 0, scale 1)."""
    return [{"first_cam": 0, "views": views, "R": np.asarray(Rs[s], np.float32), "t": np.asarray(pos[s], np.float32), "scale": np.float32(1.0)}
            for s in range(len(pos))]


def rough_instances(seed, pos, Rs, offset_mm=15.0, max_deg=6.0, views=0b111):
    """Seeded rough world starts about the true poses (fit_scenes.start): 15 mm and up to 6 degrees off."""
    out = []
    for s in range(len(pos)):
        R, t = fs.start(1000 * seed + s, pos[s], Rs[s], offset_mm, max_deg)
        out.append({"first_cam": 0, "views": views, "R": R, "t": t, "scale": np.float32(1.0)})
    return out


def errors(V, u, Vt, ut, pos):
    """Per camera: (rotation error in degrees, the worst distance in mm between where the camera and the true camera put the
    true head positions `pos` in the camera frame)."""
    out = []
    for c in range(len(V)):
        a, b = np.asarray(V[c], np.float64), np.asarray(Vt[c], np.float64)
        d = (pos @ a.T + np.asarray(u[c], np.float64)) - (pos @ b.T + np.asarray(ut[c], np.float64))
        out.append((float(fs.geodesic_deg(a, b)), float(np.sqrt((d * d).sum(axis=1)).max())))
    return out


def as_records(instances, model=0, flags=0):
    """Instance dicts as a VIEW_INSTANCE_DTYPE array."""
    from depthhead_amd._lib import VIEW_INSTANCE_DTYPE
    out = np.zeros(len(instances), VIEW_INSTANCE_DTYPE)
    for i, s in enumerate(instances):
        out[i] = (s["first_cam"], model, s["views"], np.asarray(s["R"], np.float32).reshape(9), np.asarray(s["t"], np.float32).reshape(3), s["scale"],
                  flags)
    return out
