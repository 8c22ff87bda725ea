"""The fitting rule itself (tests/fit_ref.py) on scenes rendered by the renderer's restatement: 160 x 120,
head_mesh(2) and its torso box at 12 seeded poses, noise 2, holes 0.02.  No GPU: what is held here is that the rule converges,
its exits, and the host functions of depthhead_amd.fit.  tests/test_gpu_fit.py holds the GPU to the same restatement."""
import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
from depthhead_amd import _lib, fit, render, synth

W, H = 160, 120
SEEDS = range(7000, 7012)
# The restatement's own worst case over the 24 fits below, times two for other seeds: measured 2.93 mm
# (seed 7004 from 90 mm) and 5.90 degrees (seed 7007 from 20 mm).
MAX_POS_MM, MAX_ROT_DEG = 5.9, 11.8


def run(seed, offset, deg):
    frame, K, pos, R = fs.scene(W, H, seed)
    v, _, nm = fs.head()
    R0, t0 = fs.start(seed, pos, R, offset, deg)
    R1, t1, rec = fr.fit(frame, K, v, nm, R0, t0)
    return (np.linalg.norm(t0 - pos), np.linalg.norm(t1 - pos), fs.geodesic_deg(R0, R), fs.geodesic_deg(R1, R), rec)


@pytest.mark.parametrize("seed", SEEDS)
def test_far_start_ends_closer_in_position_and_rotation(seed):
    p0, p1, r0, r1, rec = run(seed, 90.0, 25.0)
    print(f"seed {seed}: position {p0:.1f} -> {p1:.2f} mm, rotation {r0:.1f} -> {r1:.2f} deg, {rec}")
    assert rec["status"] == fr.OK and rec["points"] >= 40
    assert p1 < p0 and r1 < r0
    assert p1 <= MAX_POS_MM and r1 <= MAX_ROT_DEG


@pytest.mark.parametrize("seed", SEEDS)
def test_near_start_improves_position(seed):
    p0, p1, r0, r1, rec = run(seed, 20.0, 10.0)
    print(f"seed {seed}: position {p0:.1f} -> {p1:.2f} mm, rotation {r0:.1f} -> {r1:.2f} deg, {rec}")
    assert rec["status"] == fr.OK
    assert p1 < p0
    assert p1 <= MAX_POS_MM and r1 <= MAX_ROT_DEG


def test_rms_of_the_record():
    _, _, _, _, rec = run(7000, 20.0, 10.0)
    r = fit.rms(rec)
    assert 0.5 < r < 4.0                       # +-2 mm of uniform noise and a faceted model
    assert np.isnan(fit.rms({"points": 0, "sum_r2_fixed": 0}))


def test_vertex_normals_of_a_box_and_an_icosphere():
    v, t = synth.box_mesh((-1, -2, -3), (1, 2, 3))
    n = fit.vertex_normals(v, t)
    assert n.dtype == np.float32 and n.shape == v.shape
    assert np.allclose((n.astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6)
    assert (np.sign(n) == -np.sign(v)).all()                   # box_mesh winds inward: every corner's normal points at the centre
    assert (np.sign(fit.vertex_normals(v, t[:, ::-1])) == np.sign(v)).all()
    u, t = synth._icosphere(2)
    n = fit.vertex_normals(u, t).astype(np.float64)
    assert np.allclose((n * n).sum(axis=1), 1.0, atol=1e-6)
    assert ((n * u).sum(axis=1) > 0.999).all()                 # a sphere's normal is its radius
    assert ((fit.vertex_normals(u, t[:, ::-1]).astype(np.float64) * u).sum(axis=1) < -0.999).all()      # nothing is flipped by guessing
    hv, _, hn = fs.head()
    assert ((hn * hv).sum(axis=1) > 0).all()


def test_matrix_to_euler_inverts_euler_to_matrix():
    u = synth.SplitMix(5).uniform(60).reshape(20, 3)
    for k in range(20):
        r = np.array([360 * u[k, 0] - 180, 170 * u[k, 1] - 85, 360 * u[k, 2] - 180])
        got = fit.matrix_to_euler(render.euler_to_matrix(r))
        assert np.allclose(got, r, atol=1e-3), (r, got)        # (the matrix is f32)
    assert np.allclose(fit.matrix_to_euler(np.eye(3)), 0.0)


def test_cayley_stays_orthonormal_over_64_steps():
    u = synth.SplitMix(11).uniform(64 * 3).reshape(64, 3)
    R = np.eye(3)
    for k in range(64):
        w = 0.6 * (2.0 * u[k] - 1.0)
        R2 = fr.cayley(R, list(w))
        if k == 0:                                             # a rotation about w by 2 atan(|w| / 2)
            ang = 2.0 * np.arctan(np.linalg.norm(w) / 2.0)
            assert abs(np.degrees(ang) - fs.geodesic_deg(np.eye(3), R2)) < 1e-9
            assert np.allclose(R2 @ w, w, atol=1e-12)
        R = R2
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12


def test_early_exit_from_the_coarse_phase_and_then_from_the_full_steps_on_a_head_scene():
    """On rendered heads the default damping never reaches the early exit: the associated pixel and its integer depth change
    with the pose, and the steps level off between 0.05 and 1 mm even without noise (64 steps of 64 below).  What does reach it on
    such a scene is heavy damping: with lambda = 1e8 the first coarse step is below 1e-6 and ends the coarse phase, the fit goes
    on to the full steps, and the first of those ends it.  From the far start the full pass at the 25 mm gate finds nothing."""
    frame, K, pos, R = fs.scene(W, H, 7003)
    v, _, nm = fs.head()
    far, near = fs.start(7003, pos, R, 90.0, 25.0), fs.start(7003 + 31, pos, R, 20.0, 10.0)
    _, t1, rec = fr.fit(frame, K, v, nm, *near, prm=fr.params(lam=1e8))
    assert (rec["steps"], rec["status"]) == (2, fr.OK) and rec["points"] >= 30 and np.abs(t1 - near[1]).max() < 1e-3
    _, _, rec = fr.fit(frame, K, v, nm, *far, prm=fr.params(lam=1e8))
    assert (rec["steps"], rec["status"], rec["points"]) == (1, fr.FEW_POINTS, 0)
    _, _, rec = fr.fit(frame, K, v, nm, *near, prm=fr.params(lam=1e7))
    assert (rec["steps"], rec["status"]) == (7, fr.OK)                 # six coarse steps, none small enough; one full step that is
    clean = fs.scene(W, H, 7003, 0, 0.0)[0]
    _, _, rec = fr.fit(clean, K, v, nm, *near, prm=fr.params(coarse_iterations=32, iterations=32))
    assert (rec["steps"], rec["status"]) == (64, fr.OK)


def test_empty_frame_gives_few_points_and_the_pose_unchanged():
    v, _, nm = fs.head()
    K = synth.default_intrinsic(W, H)
    R0 = render.euler_to_matrix((3, 20, -5))
    t0 = np.array([10.0, -20.0, 900.0], np.float32)
    R1, t1, rec = fr.fit(np.zeros((H, W), np.uint16), K, v, nm, R0, t0)
    assert rec == {"points": 0, "steps": 0, "status": fr.FEW_POINTS, "sum_r2_fixed": 0}
    assert R1.tobytes() == R0.tobytes() and t1.tobytes() == t0.tobytes()


def plane_model(n=9, step=20.0):
    g = (np.arange(n) - (n - 1) / 2.0) * step
    x, y = np.meshgrid(g, g)
    pts = np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], axis=1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, -1], np.float32), (n * n, 1))
    return pts, nrm


def test_coplanar_points_seen_face_on():
    """A plane seen face-on is degenerate: every normal is (0, 0, -1), so A_00 = A_11 = 0 and J_5 = 0 before damping.  With
    lambda = 0 the 1e-9 term alone is then the pivot, and it DOES remove the singularity: the pivot is > 0.0, the matching b_a
    are zero, so x_a = 0 there and the restatement goes on (status OK, the plane moves along z onto the wall).  The same plane
    turned by a few degrees has the same null space, no longer along the axes: elimination cancels the diagonal to a pivot that
    is not > 0.0, and that is where lambda = 0 ends with SINGULAR at the first step, the pose as it was."""
    pts, nrm = plane_model()
    K = synth.default_intrinsic(W, H)
    frame = np.full((H, W), 800, np.uint16)
    zero = fr.params(coarse_iterations=4, iterations=0, lam=0.0)
    R1, t1, rec = fr.fit(frame, K, pts, nrm, np.eye(3), np.array([0.0, 0.0, 830.0], np.float32), prm=zero)
    assert rec == {"points": 81, "steps": 2, "status": fr.OK, "sum_r2_fixed": 0}
    assert t1.tolist() == [0.0, 0.0, 800.0] and R1.tobytes() == np.eye(3, dtype=np.float32).tobytes()
    t0 = np.array([0.0, 0.0, 810.0], np.float32)
    R1, t1, rec = fr.fit(frame, K, pts, nrm, np.eye(3), t0, prm=fr.params(coarse_iterations=0, iterations=3, lam=0.0))
    assert rec == {"points": 81, "steps": 2, "status": fr.OK, "sum_r2_fixed": 0} and t1.tolist() == [0.0, 0.0, 800.0]
    # without the 1e-9 term the system is singular, and the solver refuses a pivot that is zero or NaN
    assert fr.solve([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 81.0]], [0.0, 0.0, 1.0], 3) is None
    assert fr.solve([[float("nan")]], [1.0], 1) is None
    R0 = render.euler_to_matrix((0, 4, 3))
    R1, t1, rec = fr.fit(frame, K, pts, nrm, R0, t0, prm=fr.params(coarse_iterations=0, iterations=3, lam=0.0))
    assert rec["status"] == fr.SINGULAR and rec["steps"] == 0 and rec["points"] == 81 and rec["sum_r2_fixed"] > 0
    assert R1.tobytes() == R0.tobytes() and t1.tobytes() == t0.tobytes()


def test_instances_from_poses():
    poses = np.zeros(2, _lib.POSE_DTYPE)
    poses["mid_point"] = [(1, 2, 900), (-3, 4, 1000)]
    poses["rotation"] = np.radians([(5, -20, 10), (0, 0, 0)])
    inst = fit.instances_from_poses(poses, scale=1.5)
    assert inst["frame"].tolist() == [0, 1] and (inst["scale"] == 1.5).all() and inst["t"][1].tolist() == [-3, 4, 1000]
    assert np.allclose(inst["R"][0].reshape(3, 3), render.euler_to_matrix((5, -20, 10)), atol=1e-6)
    heads = np.zeros((2, 1), _lib.HEAD_DTYPE)
    heads["pose"][:, 0] = poses
    assert fit.instances_from_poses(heads, scale=1.5, frames=[0, 1]).tobytes() == inst.tobytes()
    assert np.allclose(fit.matrix_to_euler(inst["R"][0].reshape(3, 3)), (5, -20, 10), atol=1e-4)
