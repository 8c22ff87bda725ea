"""Sequences shared by the fit-tracker tests (test_fit_track_ref.py on the CPU, test_gpu_fit_tracker.py on the GPU): a head
(head_mesh(2)) and its torso box moving 12 mm and 3 degrees of yaw per step, rendered by the renderer's restatement with the
sensor model, and the forest's answer faked as the truth plus a 90 mm offset with the angles on the forest's 3-degree grid.
Every array is computed once and handed out read-only."""
import functools

import numpy as np

import fit_scenes as fs
import render_ref as rr
from depthhead_amd import _lib, render, synth, training

STEP_MM, STEP_YAW = 12.0, 3.0
BIN = 3.14159 / 60.0


def good_support(n=1):
    """Support records a detected head would give: confidence 0.1, ten windows."""
    s = np.zeros(n, _lib.SUPPORT_DTYPE)
    s["width"], s["height"], s["windows"], s["hits"], s["mass"], s["total_mass"] = 8, 8, 10, 40, 100, 1000
    return s


def fake_pose(pos, rot_deg, seed, offset_mm=90.0):
    """A dh_pose as the forest would report the head at (pos, rot_deg): the position `offset_mm` off in a seeded direction and
    rounded to integers, the angles rounded to multiples of 3.14159 / 60."""
    d = 2.0 * synth.SplitMix(700000 + seed).uniform(3) - 1.0
    d = d / np.sqrt((d * d).sum())
    p = np.zeros((), _lib.POSE_DTYPE)
    p["mid_point"] = np.round(np.asarray(pos, np.float64) + offset_mm * d)
    p["rotation"] = np.round(np.radians(np.asarray(rot_deg, np.float64)) / BIN) * BIN
    return p


@functools.lru_cache(maxsize=None)
def sequence(w, h, seed, steps=8, gone=(), K_key=None):
    """(frames [steps, h, w] u16, K, true positions [steps, 3] f64, true R [steps, 3, 3] f64, poses POSE_DTYPE [steps]) of one
    head moving STEP_MM in a seeded direction across the image and STEP_YAW degrees of yaw towards the front per step.  The
    frames listed in `gone` are empty.  K_key: a 9-tuple to render through instead of the default intrinsic matrix."""
    pos0, rot0 = training.rendered_pose(w, h, seed)
    K = synth.default_intrinsic(w, h) if K_key is None else np.asarray(K_key, np.float32).reshape(3, 3)
    u = synth.SplitMix(800000 + seed).uniform(2)
    ang = 2.0 * np.pi * u[0]
    d = np.array([np.cos(ang), 0.5 * np.sin(ang), 0.5 * (2.0 * u[1] - 1.0)])
    d = d / np.sqrt((d * d).sum())
    if (pos0[0] + steps * STEP_MM * d[0]) ** 2 > pos0[0] ** 2:           # towards the middle of the frame
        d[0] = -d[0]
    v, t, _ = fs.head()
    frames, pos, Rs = [], [], []
    poses = np.zeros(steps, _lib.POSE_DTYPE)
    for k in range(steps):
        p = pos0.astype(np.float64) + k * STEP_MM * d
        rot = rot0.astype(np.float64).copy()
        rot[training.YAW] -= np.sign(rot[training.YAW]) * STEP_YAW * k
        R = render.euler_to_matrix(rot)
        if k in gone:
            frames.append(np.zeros((h, w), np.uint16))
        else:
            items = [rr.instance(0, 0, R, p), rr.instance(0, 1, None, p, head=False)]
            frames.append(rr.render([(v, t), fs.torso()], items, 1, w, h, K, noise=2, holes=0.02, seed=seed * 100 + k)[0][0])
        pos.append(p); Rs.append(R.astype(np.float64))
        poses[k] = fake_pose(p, rot, seed * 100 + k)
    out = (np.stack(frames), K, np.stack(pos), np.stack(Rs), poses)
    for a in out:
        a.setflags(write=False)
    return out
