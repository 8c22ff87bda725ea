"""Scenes shared by the multi-view fit tests (test_view_fit_ref.py on the CPU, test_gpu_fit_views.py on the GPU): ONE head
(head_mesh(2)) at a seeded pose in the world frame and its torso box, rendered by the renderer's restatement (tests/render_ref.py)
through 2 or 3 cameras placed on an arc about the world origin, with the sensor model (noise 2, holes 0.02).  The world frame
is that of a camera at (0, 0, -d) looking along +z: x right, y down, the face looks along -z.  Every array is computed once and
handed out read-only."""
import functools

import numpy as np

import fit_scenes as fs
import render_ref as rr
from depthhead_amd import fit, render, synth

YAWS = {1: (0.0,), 2: (-35.0, 25.0), 3: (-35.0, 0.0, 35.0)}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def arc(yaws_deg, dists):
    """The rig's extrinsics (R [n, 3, 3], t [n, 3], f64, camera to world) of cameras on an arc about the world origin: camera c
    is turned by yaws_deg[c] about the world's y axis and stands dists[c] mm from the origin, which lies on its optical axis."""
    R, t = [], []
    for a, d in zip(yaws_deg, dists):
        ca, sa = np.cos(np.radians(a)), np.sin(np.radians(a))
        Rc = np.array([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]])
        R.append(Rc)
        t.append(-d * Rc[:, 2])
    return np.array(R), np.array(t)


@functools.lru_cache(maxsize=None)
def truth(seed):
    """(world position [3] f64 within 60 mm of the origin per axis, world rotation [3, 3] f64: yaw +-30, pitch +-15, roll +-10
    degrees, camera distances [3] in 700 .. 1200 mm) of scene `seed`."""
    u = synth.SplitMix(210000 + seed).uniform(9)
    pos = 60.0 * (2.0 * u[:3] - 1.0)
    rot = np.array([30.0, 15.0, 10.0]) * (2.0 * u[3:6] - 1.0)
    return _ro(pos, render.euler_to_matrix(rot).astype(np.float64), 700.0 + 500.0 * u[6:9])


def view_items(pos, R, V, u, first=0):
    """The render instances of one world-posed head (mesh 0) and its torso box (mesh 1) in the frames of cameras first ..: the
    head at (V R, V pos + u), the box turned with the camera."""
    items = []
    for c in range(len(V)):
        Vc, uc = np.asarray(V[c], np.float64), np.asarray(u[c], np.float64)
        tc = Vc @ np.asarray(pos, np.float64) + uc
        items += [(first + c, 0, Vc @ np.asarray(R, np.float64), tc, 1.0, True), (first + c, 1, Vc, tc, 1.0, False)]
    return items


@functools.lru_cache(maxsize=None)
def scene(seed, n_views=3, w=160, h=120, noise=2, holes=0.02, yaws=None):
    """(frames [n, h, w] u16, Ks [n, 3, 3] f32, V [n, 3, 3] f32, u [n, 3] f32, true world position [3] f64, true world R
    [3, 3] f64).  V, u come from fit.views_from_rig of the arc's extrinsics (yaws: YAWS[n_views] unless given; the distances
    of cameras past the third repeat the first three)."""
    pos, R, dists = truth(seed)
    yaws = YAWS[n_views] if yaws is None else yaws
    V, u = fit.views_from_rig(*arc(yaws, [dists[c % 3] for c in range(n_views)]))
    K = synth.default_intrinsic(w, h)
    v, t, _ = fs.head()
    items = [rr.instance(f, m, Rc, tc, head=hd) for f, m, Rc, tc, _, hd in view_items(pos, R, V, u)]
    frames, _ = rr.render([(v, t), fs.torso()], items, n_views, w, h, K, noise=noise, holes=holes, seed=seed)
    Ks = np.ascontiguousarray(np.broadcast_to(K, (n_views, 3, 3)))
    return _ro(frames, Ks, V, u, pos.copy(), R.copy())


def camera_pose(V, u, R, t):
    """The camera-frame pose (R [3, 3] f32, t [3] f32) of a world pose through one view."""
    V, u = np.asarray(V, np.float64), np.asarray(u, np.float64)
    return (V @ np.asarray(R, np.float64)).astype(np.float32), (V @ np.asarray(t, np.float64) + u).astype(np.float32)


start = fs.start
geodesic_deg = fs.geodesic_deg
