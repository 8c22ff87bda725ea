"""Scenes shared by the subject-tracker tests (test_subject_track_ref.py on the CPU, test_gpu_subject_tracker.py on the GPU;
DESIGN.md section 29): a gallery of ident_scenes' kind -- subjects that differ by one coefficient -- and per camera one head
that moves a little every step, splatted from the model of the subject the camera shows (cheap at any size), with the forest's
answer faked as fit_track_scenes fakes it.  A stranger is a head of the same mesh at a coefficient no subject of the gallery
has.  Every array is computed once and handed out read-only."""
import functools

import numpy as np

import fit_track_scenes as fts
import ident_scenes as isc
import subjects_ref as sb
import surface_ref as su
import surface_scenes as us
from depthhead_amd import _lib, render, synth

STEP_MM, STEP_YAW = 6.0, 2.0
STRANGER = -1                     # `who` of a camera that shows nobody of the gallery
STRANGER_COEFF = 1.6              # far outside the gallery's +-0.4


@functools.lru_cache(maxsize=None)
def mesh(name):
    """ident_scenes.mesh, and "lathe<rings>x<segments>": a closed surface of revolution of rings * segments + 2 vertices with the
    same kind of field (lathe31x33 has 1025 vertices, one more than the fit stages in LDS)."""
    if not name.startswith("lathe"):
        return isc.mesh(name)
    import subjects_scenes as sc
    rings, segments = (int(x) for x in name[5:].split("x"))
    v, t = sc.lathe_mesh(rings, segments)
    return v, t, (0.5 * (v * np.array([1.0, -0.5, 0.0], np.float32))[None] + 0.1 * sc.seeded_fields(v, 1, 40 + len(v))).astype(np.float32)


def restated_set(name, n_subjects, surface=False):
    """A fresh restated set of the gallery `name` with ident_scenes' coefficients (and, for a surface set, its bumps)."""
    v, t, B = mesh(name)
    st = su.Set(v, t, B, n_subjects, max_offset=16.0) if surface else sb.Set(v, t, B, n_subjects)
    st.set_coeffs(isc.coefficients(n_subjects))
    if surface:
        for s in range(n_subjects):
            st.set_offsets(s, us.bump(v, (7 * s + 3) % len(v), 5.0 - 2.0 * (s % 3), 0.2 * float(np.ptp(v, axis=0).max())))
    return v, t, B, st


@functools.lru_cache(maxsize=None)
def generic(name):
    """(points, normals) of the gallery's base mesh: the generic model."""
    v, t, _ = mesh(name)
    n, _ = sb.normals(v, t)
    v, n = v.copy(), n.copy()
    v.setflags(write=False); n.setflags(write=False)
    return v, n


@functools.lru_cache(maxsize=None)
def sequence(name, n_subjects, w, h, who, steps, seed=3, gone=(), K_keys=None, z=800.0, surface=False):
    """(frames [steps, n, h, w] u16, Ks [n, 3, 3], true t [steps, n, 3], true R [steps, n, 3, 3], poses POSE_DTYPE [steps, n]):
    camera c shows subject who[c] of the gallery (STRANGER: the stranger) moving STEP_MM along a seeded direction and STEP_YAW
    degrees of yaw per step.  gone: (step, camera) pairs whose frame is empty.  K_keys: per camera a 9-tuple or None."""
    v, t, B, st = restated_set(name, n_subjects, surface)
    strange = sb.points(v, B, [STRANGER_COEFF])
    n = len(who)
    K0 = synth.default_intrinsic(w, h)
    Ks = np.stack([K0 if not K_keys or K_keys[c] is None else np.asarray(K_keys[c], np.float32).reshape(3, 3) for c in range(n)]).astype(np.float32)
    frames = np.zeros((steps, n, h, w), np.uint16)
    ts, Rs = np.zeros((steps, n, 3)), np.zeros((steps, n, 3, 3))
    poses = np.zeros((steps, n), _lib.POSE_DTYPE)
    for c in range(n):
        u = synth.SplitMix(900000 + 100 * seed + c).uniform(6)
        rot0 = (2.0 * u[:3] - 1.0) * 10.0
        t0 = np.array([(2.0 * u[3] - 1.0) * 0.06 * z, (2.0 * u[4] - 1.0) * 0.04 * z, z + 40.0 * u[5]])
        ang = 2.0 * np.pi * u[0]
        d = np.array([np.cos(ang), 0.5 * np.sin(ang), 0.3])
        d = d / np.sqrt((d * d).sum())
        if t0[0] * d[0] > 0:                                             # towards the middle of the frame
            d[0] = -d[0]
        pts = strange if who[c] == STRANGER else st.pts[who[c]]
        for k in range(steps):
            p = t0 + k * STEP_MM * d
            rot = rot0.copy()
            rot[1] += STEP_YAW * k
            R = render.euler_to_matrix(rot)
            ts[k, c], Rs[k, c] = p, R
            if (k, c) not in gone:
                frames[k, c] = us.splat(pts, Ks[c], us.instance(c, R, p), w, h, seed=seed * 1000 + 10 * k + c)
            poses[k, c] = fts.fake_pose(p, rot, seed * 1000 + 10 * k + c, offset_mm=20.0)
    out = (frames, Ks, ts, Rs, poses)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the evaluation: section 27's gallery, each of its people moving as fit_track_scenes.sequence moves its head
EVAL_STEPS = 8


@functools.lru_cache(maxsize=None)
def eval_sequence(seed, steps=EVAL_STEPS, salt=0):
    """(frames [steps, h, w] u16, K, true positions [steps, 3], true R [steps, 3, 3], poses POSE_DTYPE [steps]) of section 26's
    subject `seed` -- the generic head with its two bumps, over the torso box -- moving fit_track_scenes.STEP_MM and STEP_YAW a
    step from a start no enrolment frame has (rendered_pose of 5000 * seed + salt), rendered with the sensor model."""
    import fit_scenes as fs
    import render_ref as rr
    from depthhead_amd import training
    w, h = us.EVAL_W, us.EVAL_H
    v, t, n, _ = us.eval_generic()
    sv = (v.astype(np.float64) + us.eval_bumps(seed)[:, None] * n.astype(np.float64)).astype(np.float32)
    K = synth.default_intrinsic(w, h)
    key = 5000 * seed + salt
    pos0, rot0 = training.rendered_pose(w, h, key)
    u = synth.SplitMix(800000 + key).uniform(2)
    ang = 2.0 * np.pi * u[0]
    d = np.array([np.cos(ang), 0.5 * np.sin(ang), 0.5 * (2.0 * u[1] - 1.0)])
    d = d / np.sqrt((d * d).sum())
    if (pos0[0] + steps * fts.STEP_MM * d[0]) ** 2 > pos0[0] ** 2:          # towards the middle of the frame
        d[0] = -d[0]
    frames, pos, Rs = [], [], []
    poses = np.zeros(steps, _lib.POSE_DTYPE)
    for k in range(steps):
        p = pos0.astype(np.float64) + k * fts.STEP_MM * d
        rot = rot0.astype(np.float64).copy()
        rot[training.YAW] -= np.sign(rot[training.YAW]) * fts.STEP_YAW * k
        R = render.euler_to_matrix(rot)
        items = [rr.instance(0, 0, R, p), rr.instance(0, 1, None, p, head=False)]
        frames.append(rr.render([(sv, t), fs.torso()], items, 1, w, h, K, noise=2, holes=0.02, seed=key * 100 + k)[0][0])
        pos.append(p); Rs.append(R.astype(np.float64))
        poses[k] = fts.fake_pose(p, rot, key * 100 + k)
    out = (np.stack(frames), K, np.stack(pos), np.stack(Rs), poses)
    for a in out:
        a.setflags(write=False)
    return out
