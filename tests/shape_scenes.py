"""Scenes shared by the shape tests (test_shape_ref.py on the CPU, test_gpu_fit_shape.py on the GPU), built like fit_scenes.scene:
a SUBJECT whose head is synth.head_mesh(2) stretched by (1.08, 0.93, 1.06) -- in the basis of synth.head_basis the coefficients
C_TRUE -- with its torso box, at eight seeded poses, rendered by the renderer's restatement with the sensor model.  The GENERIC
model is head_mesh(2) itself.  Every array is computed once and handed out read-only."""
import functools

import numpy as np

import fit_scenes as fs
import render_ref as rr
from depthhead_amd import fit, render, synth, training

C_TRUE = (0.08, -0.07, 0.06, 0.0)      # the stretch (1.08, 0.93, 1.06); the nose as the generic head's
POSES = 8


@functools.lru_cache(maxsize=None)
def generic():
    """(verts, tris, normals, basis [4, n, 3]) of the generic model."""
    v, t, n = fs.head(2)
    return fs._ro(v, t, n, synth.head_basis(v))


@functools.lru_cache(maxsize=None)
def subject_mesh(c_true=C_TRUE):
    v, t, _, B = generic()
    sv = fit.deform(v, B, c_true)
    return fs._ro(sv, t, fit.vertex_normals(sv, t))


@functools.lru_cache(maxsize=None)
def subject(w, h, seed, c_true=C_TRUE, poses=POSES, noise=2, holes=0.02):
    """(frames [poses, h, w] u16, K, true positions [poses, 3] f64, true R [poses, 3, 3] f64) of subject `seed`: pose i is
    training.rendered_pose(w, h, 1000 * seed + i), frame i holds the subject's head there and its torso box."""
    K = synth.default_intrinsic(w, h)
    sv, t, _ = subject_mesh(c_true)
    items, pos, Rs = [], [], []
    for i in range(poses):
        p, rot = training.rendered_pose(w, h, 1000 * seed + i)
        R = render.euler_to_matrix(rot)
        items += [rr.instance(i, 0, R, p), rr.instance(i, 1, None, p, head=False)]
        pos.append(p.astype(np.float64))
        Rs.append(R.astype(np.float64))
    frames, _ = rr.render([(sv, t), fs.torso()], items, poses, w, h, K, noise=noise, holes=holes, seed=seed)
    return fs._ro(frames, K, np.array(pos), np.array(Rs))


def true_instances(pos, Rs):
    """The true poses as instance dicts for shape_ref (frame i, scale 1)."""
    return [{"frame": i, "R": np.asarray(Rs[i], np.float32), "t": np.asarray(pos[i], np.float32), "scale": np.float32(1.0)}
            for i in range(len(pos))]


def rough_instances(seed, pos, Rs, offset_mm=15.0, max_deg=6.0):
    """Seeded rough starts about the true poses (fit_scenes.start)."""
    out = []
    for i in range(len(pos)):
        R, t = fs.start(1000 * seed + i, pos[i], Rs[i], offset_mm, max_deg)
        out.append({"frame": i, "R": R, "t": t, "scale": np.float32(1.0)})
    return out


def as_records(instances):
    """Instance dicts as a RENDER_INSTANCE_DTYPE array (mesh 0, flags 0)."""
    from depthhead_amd._lib import RENDER_INSTANCE_DTYPE
    out = np.zeros(len(instances), RENDER_INSTANCE_DTYPE)
    for i, s in enumerate(instances):
        out[i] = (s["frame"], 0, np.asarray(s["R"], np.float32).reshape(9), s["t"], s["scale"], 0)
    return out
