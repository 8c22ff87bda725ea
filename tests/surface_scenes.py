"""Meshes and scenes shared by the surface tests (test_surface_ref.py on the CPU, test_gpu_surface.py on the GPU; DESIGN.md section
26): a strip mesh of any vertex count, depth frames splatted from a displaced mesh (cheap at any size, so a test can place a bump
where it wants it), seeded poses, and the evaluation's subjects -- head_mesh(3) with bumps outside head_basis's span, rendered by
the renderer's restatement.  What is expensive is computed once."""
import functools

import numpy as np

import fit_scenes as fs
import render_ref as rr
import shape_scenes as ss
import subjects_ref as sb
from depthhead_amd import render, synth, training


def strip_mesh(n, step=0.4, half_width=30.0):
    """A curved zigzag strip of exactly n >= 3 vertices and n - 2 triangles along x, facing the camera (normals toward -z), no
    vertex with a zero normal: vertex i at x = step * (i - n / 2), y = +-half_width alternating, z a shallow bowl with a ripple."""
    i = np.arange(n, dtype=np.float64)
    x = step * (i - n / 2.0)
    y = np.where(i % 2 == 0, -half_width, half_width)
    z = 2e-5 * x * x + 0.5 * np.sin(0.05 * i)
    verts = np.stack([x, y, z], axis=1).astype(np.float32)
    k = np.arange(n - 2)
    tris = np.where((k % 2 == 0)[:, None], np.stack([k, k + 2, k + 1], axis=1), np.stack([k, k + 1, k + 2], axis=1)).astype(np.uint32)
    nrm, zero = sb.normals(verts, tris)
    if (nrm[:, 2] > 0).all():
        tris = np.ascontiguousarray(tris[:, ::-1])
        nrm, zero = sb.normals(verts, tris)
    assert zero == 0 and (nrm[:, 2] < 0).all()
    return verts, tris


def pose(seed, w, h, z=800.0, spread=0.25, max_deg=12.0):
    """A seeded pose in front of a w x h camera: (R [3, 3] f32, t [3] f32)."""
    u = synth.SplitMix(seed).uniform(6)
    rot = (2.0 * u[:3] - 1.0) * max_deg
    t = np.array([(2.0 * u[3] - 1.0) * spread * z * w / (2.0 * w), (2.0 * u[4] - 1.0) * spread * z * h / (2.0 * w), z + 60.0 * u[5]])
    return render.euler_to_matrix(rot).astype(np.float32), t.astype(np.float32)


def instance(frame, R, t, scale=1.0):
    return {"frame": int(frame), "R": np.asarray(R, np.float32).reshape(3, 3), "t": np.asarray(t, np.float32).reshape(3), "scale": np.float32(scale)}


def splat(verts, K, inst, w, h, seed=0, noise=2):
    """One u16 frame: every vertex of `verts` [n, 3] posed by `inst`, its depth written to the 3 x 3 pixels around its projection
    (the nearest wins), seeded noise of +-`noise` mm added where something was written; 0 elsewhere."""
    R, t, s = inst["R"].astype(np.float64), inst["t"].astype(np.float64), float(inst["scale"])
    p = (np.asarray(verts, np.float64) * s) @ R.T + t
    Kd = np.asarray(K, np.float64).reshape(3, 3)
    q = p @ Kd.T
    frame = np.full((h, w), 65535, np.int64)
    ok = p[:, 2] >= 1.0
    x, y = np.floor(q[ok, 0] / q[ok, 2]).astype(np.int64), np.floor(q[ok, 1] / q[ok, 2]).astype(np.int64)
    z = np.rint(p[ok, 2]).astype(np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            xx, yy = x + dx, y + dy
            inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            np.minimum.at(frame, (yy[inside], xx[inside]), z[inside])
    hit = frame < 65535
    jitter = (synth.SplitMix(1000 + seed).uniform(w * h).reshape(h, w) * (2 * noise + 1)).astype(np.int64) - noise
    return np.where(hit, np.clip(frame + jitter, 1, 65534), 0).astype(np.uint16)


def splat_scene(verts, nb, disp, w, h, n_frames, seed, scale=1.0, **pose_kw):
    """(frames [n_frames, h, w] u16, K, instances): the mesh displaced by disp [n] mm along nb, at `n_frames` seeded poses."""
    K = synth.default_intrinsic(w, h)
    target = np.asarray(verts, np.float64) + np.asarray(disp, np.float64)[:, None] * np.asarray(nb, np.float64)
    inst = [instance(f, *pose(seed * 100 + f, w, h, **pose_kw), scale=scale) for f in range(n_frames)]
    frames = np.stack([splat(target, K, it, w, h, seed=seed * 100 + f) for f, it in enumerate(inst)])
    return frames, K, inst


def bump(verts, centre, height, sigma):
    """A Gaussian bump [n] (mm) about vertex `centre`."""
    v = np.asarray(verts, np.float64)
    d2 = ((v - v[centre]) ** 2).sum(axis=1)
    return height * np.exp(-d2 / (2.0 * sigma * sigma))


# ---- the evaluation's subjects: head_mesh(3) with two bumps that head_basis cannot express
EVAL_W, EVAL_H, EVAL_SEEDS = 320, 240, (12, 13, 14)


@functools.lru_cache(maxsize=None)
def eval_generic():
    """(verts, tris, normals, basis) of the generic 642-point head."""
    v, t, n = fs.head(3)
    return fs._ro(v, t, n, synth.head_basis(v))


@functools.lru_cache(maxsize=None)
def eval_bumps(seed):
    """The subject's true displacement [n] (mm) along the generic head's normals: +8.5 and -6 mm bumps of 22 mm sigma about two
    seeded vertices of the face (the half that looks at the camera)."""
    v, _, n, _ = eval_generic()
    face = np.flatnonzero(n[:, 2] < -0.5)
    u = synth.SplitMix(70 + seed).uniform(2)
    a, b = face[int(u[0] * len(face))], face[int(u[1] * len(face))]
    return fs._ro(bump(v, a, 8.5, 22.0) + bump(v, b, -6.0, 22.0))[0]


@functools.lru_cache(maxsize=None)
def eval_subject(seed, w=EVAL_W, h=EVAL_H, poses=8, noise=2, holes=0.02):
    """(frames [poses, h, w], K, true positions, true R) of subject `seed`, built as shape_scenes.subject builds its own."""
    v, t, n, _ = eval_generic()
    sv = (v.astype(np.float64) + eval_bumps(seed)[:, None] * n.astype(np.float64)).astype(np.float32)
    K = synth.default_intrinsic(w, h)
    items, pos, Rs = [], [], []
    for i in range(poses):
        p, rot = training.rendered_pose(w, h, 1000 * seed + i)
        R = render.euler_to_matrix(rot)
        items += [rr.instance(i, 0, R, p), rr.instance(i, 1, None, p, head=False)]
        pos.append(p.astype(np.float64))
        Rs.append(R.astype(np.float64))
    frames, _ = rr.render([(sv, t), fs.torso()], items, poses, w, h, K, noise=noise, holes=holes, seed=seed)
    return fs._ro(frames, K, np.array(pos), np.array(Rs))


def eval_starts(seed, pos, Rs):
    return ss.rough_instances(seed, pos, Rs)
