"""Scenes shared by the multi-view shape tests (test_shape_views_ref.py on the CPU, test_gpu_fit_shape_views.py on the GPU):
section 20's stretched SUBJECT (shape_scenes.subject_mesh: head_mesh(2) stretched by (1.08, 0.93, 1.06)) with its torso box,
seen by section 21's arc cameras (view_fit_scenes.arc: -35, 0 and +35 degrees about the world origin) at several SETS, one
seeded world pose each, rendered by the renderer's restatement with the sensor model (noise 2, holes 0.02).  The rig stands
still: its camera distances are those of the subject's first pose.  Every array is computed once and handed out read-only."""
import functools

import numpy as np

import fit_scenes as fs
import render_ref as rr
import shape_scenes as ss
import view_fit_scenes as vs
from depthhead_amd import fit, synth

YAWS = (-35.0, 0.0, 35.0)
MIDDLE = 1                              # the camera at yaw 0
C_TRUE = ss.C_TRUE


@functools.lru_cache(maxsize=None)
def subject(seed, n_sets=4, w=160, h=120, c_true=C_TRUE, noise=2, holes=0.02):
    """(frames [n_sets, 3, h, w] u16, Ks [3, 3, 3] f32, V [3, 3, 3] f32, u [3, 3] f32, true world positions [n_sets, 3] f64, true
    world R [n_sets, 3, 3] f64) of subject `seed`: set s holds the subject at view_fit_scenes.truth(1000 * seed + s)."""
    dists = vs.truth(1000 * seed)[2]
    V, u = fit.views_from_rig(*vs.arc(YAWS, dists))
    K = synth.default_intrinsic(w, h)
    sv, t, _ = ss.subject_mesh(c_true)
    n = len(YAWS)
    items, pos, Rs = [], [], []
    for s in range(n_sets):
        p, R, _ = vs.truth(1000 * seed + s)
        items += [rr.instance(f, m, Rc, tc, head=hd) for f, m, Rc, tc, _, hd in vs.view_items(p, R, V, u, first=s * n)]
        pos.append(p.copy())
        Rs.append(R.copy())
    frames, _ = rr.render([(sv, t), fs.torso()], items, n_sets * n, w, h, K, noise=noise, holes=holes, seed=seed)
    Ks = np.ascontiguousarray(np.broadcast_to(K, (n, 3, 3)))
    return vs._ro(frames.reshape(n_sets, n, h, w), Ks, V, u, np.array(pos), np.array(Rs))


def true_instances(pos, Rs, views=0b111):
    """The true world poses as instance dicts (set s is instance s; first_cam 0, scale 1)."""
    return [{"first_cam": 0, "views": views, "R": np.asarray(Rs[s], np.float32), "t": np.asarray(pos[s], np.float32), "scale": np.float32(1.0)}
            for s in range(len(pos))]


def rough_instances(seed, pos, Rs, offset_mm=15.0, max_deg=6.0, views=0b111):
    """Seeded rough world starts about the true poses (fit_scenes.start), section 20's 15 mm and up to 6 degrees off."""
    out = []
    for s in range(len(pos)):
        R, t = fs.start(1000 * seed + s, pos[s], Rs[s], offset_mm, max_deg)
        out.append({"first_cam": 0, "views": views, "R": R, "t": t, "scale": np.float32(1.0)})
    return out


def single_view(instances, V, u, cam=MIDDLE):
    """The camera-frame instance dicts (frame s for instance s) of world instances seen through camera `cam` alone."""
    out = []
    for s, it in enumerate(instances):
        R, t = vs.camera_pose(V[cam], u[cam], it["R"], it["t"])
        out.append({"frame": s, "R": R, "t": t, "scale": it["scale"]})
    return out


def as_records(instances, model=0, flags=0):
    """Instance dicts as a VIEW_INSTANCE_DTYPE array."""
    from depthhead_amd._lib import VIEW_INSTANCE_DTYPE
    out = np.zeros(len(instances), VIEW_INSTANCE_DTYPE)
    for i, s in enumerate(instances):
        out[i] = (s["first_cam"], model, s["views"], np.asarray(s["R"], np.float32).reshape(9), np.asarray(s["t"], np.float32).reshape(3), s["scale"],
                  flags)
    return out
