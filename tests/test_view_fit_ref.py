"""The multi-view fitting rule itself (tests/view_fit_ref.py) on scenes rendered by the renderer's
restatement: one world-posed head_mesh(2) and its torso box seen by 2 or 3 cameras on an arc (tests/view_fit_scenes.py), 160 x
120, noise 2, holes 0.02.  No GPU: what is held here is that one view through the identity IS section 18's fit, that the world
row is the right Jacobian, the exits, and how well the rule converges.  tests/test_gpu_fit_views.py holds the GPU to the same
restatement."""
import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import view_fit_ref as vr
import view_fit_scenes as vs
from depthhead_amd import render, synth

W, H = 160, 120
EYE, ZERO = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)
# The restatement's own worst case over seeds 7000 .. 7011 (three views, starts 90 mm and up to 25 degrees per axis off), times
# two for the OTHER seeds below: measured 1.76 mm (seed 7006) and 2.81 degrees (seed 7004).
MAX_POS_MM, MAX_ROT_DEG = 3.52, 5.62
OTHER_SEEDS = range(7100, 7112)


def model():
    v, _, nm = fs.head()
    return v, nm


@pytest.mark.parametrize("seed,offset,deg,prm", [(7000, 90.0, 25.0, None), (7003, 20.0, 10.0, None),
                                                 (7005, 40.0, 15.0, fr.params(3, 5, (200.0, 40.0), 0.0, 6)),
                                                 (7003, 20.0, 10.0, fr.params(lam=1e8))])
def test_one_view_through_the_identity_is_the_single_view_fit_bit_for_bit(seed, offset, deg, prm):
    frame, K, pos, R = fs.scene(W, H, seed)
    v, nm = model()
    R0, t0 = fs.start(seed, pos, R, offset, deg)
    R1, t1, rec = fr.fit(frame, K, v, nm, R0, t0, prm=prm)
    R2, t2, vrec = vr.fit(frame[None], K[None], EYE, ZERO, 0, 1, v, nm, R0, t0, prm=prm)
    assert R1.tobytes() == R2.tobytes() and t1.tobytes() == t2.tobytes()
    assert {k: vrec[k] for k in rec} == rec and vrec["views_used"] == (1 if rec["points"] else 0)
    # ... and every sum of a pass, not only what the schedule makes of them
    Rd, td = R0.astype(np.float64), t0.astype(np.float64)
    A, b, e, count = fr.one_pass(frame, K, v, nm, 1.0, Rd, td, 120.0)
    assert vr.one_pass(frame[None], K[None], EYE, ZERO, 0, 1, v, nm, 1.0, Rd, td, 120.0) == (A, b, e, count, 1)


@pytest.mark.parametrize("seed", (7000, 7004, 7009))
def test_one_view_through_a_turned_camera_is_the_single_view_fit_mapped_back(seed):
    """A sanity check on the world row J = (V^T nrm, V^T m), not a parity claim: the world-frame fit through one camera at (V, u)
    and section 18's fit of the same frame from the same start in that camera's frame.  With lambda = 0 the two systems are
    each other's rotation (the 1e-9 term is a multiple of the identity), so the fits walk the same path up to the f32 rounding
    of the camera-frame start and f64 rounding.  Observed over three seeds and three cameras: the same points, steps and status,
    at most 6.0e-4 mm in t and 3.9e-6 in an element of R once mapped back and rounded to f32 (one f32 ulp at 1000 mm is 6.1e-5
    mm; a point that changes its pixel moves the answer by more than rounding does).  Held at four times that.  With the
    default lambda = 1e-3 this does NOT hold and is not asserted: the relative damping A_aa * (1 + lambda) depends on the frame the
    rows are written in, the steps differ by 1e-3 of their length, the associations drift apart and the two fits end up to 1.9 mm
    and 6 degrees from each other -- both as close to the truth as the other."""
    frames, Ks, V, u, pos, R = vs.scene(seed, 3)
    v, nm = model()
    R0, t0 = vs.start(seed, pos, R, 90.0, 25.0)
    prm = fr.params(lam=0.0)
    for c in range(3):
        Rw, tw, vrec = vr.fit(frames, Ks, V, u, c, 1, v, nm, R0, t0, prm=prm)
        Rc0, tc0 = vs.camera_pose(V[c], u[c], R0, t0)
        Rc, tc, rec = fr.fit(frames[c], Ks[c], v, nm, Rc0, tc0, prm=prm)
        Rm, tm = vs.camera_pose(V[c], u[c], Rw, tw)
        dt, dR = np.abs(tm.astype(np.float64) - tc).max(), np.abs(Rm.astype(np.float64) - Rc).max()
        print(f"seed {seed} camera {c}: |dt| {dt:.3g} mm, |dR| {dR:.3g}, {vrec}")
        assert (vrec["points"], vrec["steps"], vrec["status"]) == (rec["points"], rec["steps"], rec["status"]) and vrec["views_used"] == 1
        assert dt <= 2.4e-3 and dR <= 1.6e-5


def test_world_row_is_the_camera_row_turned_by_V():
    """The Jacobian itself, with a bound that is derived: at the same composite pose the same points pass, and the world sums
    are the camera sums turned by B = diag(V, V): A_w = B^T A_c B, b_w = B^T b_c.  Every term of a sum loses less than one unit
    of 2^-20 to its truncating cast, and an element of B^T A_c B mixes at most nine of A_c's with weights below one: at most
    (1 + 9) * count units between the two (and (1 + 3) * count for b); f64 rounding of sums this size is below one unit."""
    frames, Ks, V, u, pos, R = vs.scene(7004, 3)
    v, nm = model()
    R0, t0 = vs.start(7004, pos, R, 20.0, 10.0)
    for c in range(3):
        Vd, ud = V[c].astype(np.float64), u[c].astype(np.float64)
        Rv, tv = vr.composite(Vd, ud, R0.astype(np.float64), t0.astype(np.float64))
        Aw, bw, ew, cw, _ = vr.one_pass(frames, Ks, V, u, c, 1, v, nm, 1.0, R0.astype(np.float64), t0.astype(np.float64), 120.0)
        Ac, bc, ec, cc = fr.one_pass(frames[c], Ks[c], v, nm, 1.0, Rv, tv, 120.0)
        assert (ew, cw) == (ec, cc) and cc >= 40
        M = np.zeros((6, 6))
        for (a, b), x in zip(fr.PAIRS, Ac):
            M[a, b] = M[b, a] = float(x)
        B = np.zeros((6, 6))
        B[:3, :3] = B[3:, 3:] = Vd
        Mw = B.T @ M @ B
        for (a, b), x in zip(fr.PAIRS, Aw):
            assert abs(float(x) - Mw[a, b]) <= 10 * cc + 1, (c, a, b)
        assert (np.abs(np.array([float(x) for x in bw]) - B.T @ np.array([float(x) for x in bc])) <= 4 * cc + 1).all()


def errors(seed, n_views=3):
    """(multi-view position error mm, rotation error degrees, the single-view fits' position errors, rotation errors) from the
    far start: the same frames, each fitted alone through its own camera from the same start."""
    frames, Ks, V, u, pos, R = vs.scene(seed, n_views)
    v, nm = model()
    R0, t0 = vs.start(seed, pos, R, 90.0, 25.0)
    R1, t1, rec = vr.fit(frames, Ks, V, u, 0, (1 << n_views) - 1, v, nm, R0, t0)
    assert rec["status"] == vr.OK and rec["views_used"] == (1 << n_views) - 1 and rec["points"] >= 40 * n_views
    assert np.linalg.norm(t1 - pos) < np.linalg.norm(t0 - pos) and vs.geodesic_deg(R1, R) < vs.geodesic_deg(R0, R)
    sp, sr = [], []
    for c in range(n_views):
        Rc, tc, _ = fr.fit(frames[c], Ks[c], v, nm, *vs.camera_pose(V[c], u[c], R0, t0))
        Vc = V[c].astype(np.float64)
        sp.append(float(np.linalg.norm(tc - (Vc @ pos + u[c]))))
        sr.append(vs.geodesic_deg(Rc, Vc @ R))
    return float(np.linalg.norm(t1 - pos)), vs.geodesic_deg(R1, R), sp, sr


def test_quality_on_other_seeds_against_the_single_view_fits_of_the_same_frames():
    """Measured on seeds 7000 .. 7011: three views end at 1.16 mm and 1.55 degrees on average (worst 1.76
    mm, 2.81 degrees); the 36 single-view fits of the same frames at 1.51 mm and 2.50 degrees on average, the BEST of each
    scene's three at 1.11 mm and 1.29 degrees.  So the multi-view fit is better than a single view taken at random and not
    better than the best one picked with the truth in hand (lower rotation error on 5 of 12 scenes): only the former is
    asserted, on the mean over the other seeds, next to the bounds at twice the measured worst case."""
    rows = [errors(seed) for seed in OTHER_SEEDS]
    for seed, (mp, mr, sp, sr) in zip(OTHER_SEEDS, rows):
        print(f"seed {seed}: multi {mp:.2f} mm {mr:.2f} deg; single {np.round(sp, 2).tolist()} mm {np.round(sr, 2).tolist()} deg")
        assert mp <= MAX_POS_MM and mr <= MAX_ROT_DEG, seed
    multi_rot, single_rot = np.mean([r[1] for r in rows]), np.mean([x for r in rows for x in r[3]])
    multi_pos, single_pos = np.mean([r[0] for r in rows]), np.mean([x for r in rows for x in r[2]])
    print(f"mean: multi {multi_pos:.2f} mm {multi_rot:.2f} deg, single {single_pos:.2f} mm {single_rot:.2f} deg")
    assert multi_rot < single_rot and multi_pos < single_pos


def test_two_views_converge_too():
    mp, mr, _, _ = errors(7101, 2)
    assert mp <= MAX_POS_MM and mr <= 2.0 * 3.42          # two views, seeds 7000 .. 7011: worst 1.76 mm, 3.42 degrees


def test_empty_frames_give_few_points_and_the_pose_unchanged():
    frames, Ks, V, u, pos, R = vs.scene(7000, 3)
    v, nm = model()
    R0, t0 = vs.start(7000, pos, R, 20.0, 10.0)
    R1, t1, rec = vr.fit(np.zeros_like(frames), Ks, V, u, 0, 7, v, nm, R0, t0)
    assert rec == {"points": 0, "steps": 0, "status": vr.FEW_POINTS, "sum_r2_fixed": 0, "views_used": 0}
    assert R1.tobytes() == R0.tobytes() and t1.tobytes() == t0.tobytes()


def test_an_empty_view_beside_two_that_see_the_head():
    frames, Ks, V, u, pos, R = vs.scene(7000, 3)
    v, nm = model()
    R0, t0 = vs.start(7000, pos, R, 90.0, 25.0)
    holed = frames.copy()
    holed[1] = 0
    R1, t1, rec = vr.fit(holed, Ks, V, u, 0, 7, v, nm, R0, t0)
    assert rec["status"] == vr.OK and rec["views_used"] == 0b101 and rec["steps"] == 20
    assert np.linalg.norm(t1 - pos) <= MAX_POS_MM and vs.geodesic_deg(R1, R) <= MAX_ROT_DEG
    # the empty view adds nothing: the fit equals the one that never named it
    R2, t2, rec2 = vr.fit(frames, Ks, V, u, 0, 0b101, v, nm, R0, t0)
    assert R1.tobytes() == R2.tobytes() and t1.tobytes() == t2.tobytes() and rec == rec2


def test_min_points_counts_all_views_together():
    frames, Ks, V, u, pos, R = vs.scene(7000, 3)
    v, nm = model()
    R0, t0 = vs.start(7000 + 31, pos, R, 20.0, 10.0)
    Rd, td = R0.astype(np.float64), t0.astype(np.float64)
    each = [vr.one_pass(frames, Ks, V, u, c, 1, v, nm, 1.0, Rd, td, 120.0)[3] for c in range(3)]
    total = vr.one_pass(frames, Ks, V, u, 0, 7, v, nm, 1.0, Rd, td, 120.0)[3]
    assert total == sum(each) and max(each) < total
    _, _, rec = vr.fit(frames, Ks, V, u, 0, 7, v, nm, R0, t0, prm=fr.params(min_points=total))
    assert rec["status"] == vr.OK and rec["steps"] >= 1        # no single view reaches it; together they do, in the first pass
    _, _, rec = vr.fit(frames, Ks, V, u, 0, 7, v, nm, R0, t0, prm=fr.params(min_points=total + 1))
    assert (rec["status"], rec["steps"]) == (vr.FEW_POINTS, 0)


def test_both_early_exits():
    """Section 18's heavy damping on a three-view scene: with lambda = 1e8 the first coarse step is below 1e-6 and ends the
    coarse phase, and the first full step ends the fit (2 steps); with 1e7 all six coarse steps run and the first full step
    ends it (7 steps)."""
    frames, Ks, V, u, pos, R = vs.scene(7003, 3)
    v, nm = model()
    near = vs.start(7003 + 31, pos, R, 20.0, 10.0)
    _, t1, rec = vr.fit(frames, Ks, V, u, 0, 7, v, nm, *near, prm=fr.params(lam=1e8))
    assert (rec["steps"], rec["status"]) == (2, vr.OK) and rec["points"] >= 90 and np.abs(t1 - near[1]).max() < 1e-3
    _, _, rec = vr.fit(frames, Ks, V, u, 0, 7, v, nm, *near, prm=fr.params(lam=1e7))
    assert (rec["steps"], rec["status"]) == (7, vr.OK)


def test_singular_exit():
    """Section 18's plane before a wall, through a turned camera and beside an empty view: the null space of a plane is the
    same in the world frame, so lambda = 0 ends with SINGULAR at the first step and the pose as it was."""
    g = (np.arange(9) - 4.0) * 20.0
    x, y = np.meshgrid(g, g)
    pts = np.stack([x.ravel(), y.ravel(), np.zeros(81)], axis=1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, -1], np.float32), (81, 1))
    K = synth.default_intrinsic(W, H)
    V, u = (a.copy() for a in vs.scene(7000, 3)[2:4])
    frames = np.zeros((3, H, W), np.uint16)
    frames[2] = 800
    Rc0, tc0 = render.euler_to_matrix((0, 4, 3)).astype(np.float64), np.array([0.0, 0.0, 810.0])
    Vd, ud = V[2].astype(np.float64), u[2].astype(np.float64)
    R0, t0 = (Vd.T @ Rc0).astype(np.float32), (Vd.T @ (tc0 - ud)).astype(np.float32)      # the world pose camera 2 sees at (Rc0, tc0)
    prm = fr.params(coarse_iterations=0, iterations=3, lam=0.0)
    R1, t1, rec = vr.fit(frames, np.stack([K] * 3), V, u, 0, 0b110, pts, nrm, R0, t0, prm=prm)
    assert rec["status"] == vr.SINGULAR and rec["steps"] == 0 and rec["points"] == 81 and rec["views_used"] == 0b100
    assert R1.tobytes() == R0.tobytes() and t1.tobytes() == t0.tobytes()
