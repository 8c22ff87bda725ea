"""The fit tracker's rule on the CPU: tests/fit_track_ref.py against scenes whose answer is known --
tests/fit_track_scenes.py's head moving 12 mm and 3 degrees of yaw per step over 160x120 frames, the forest's poses faked as
the truth plus 90 mm.  The angle table comes from the library (dh_fit_tracker_angles needs no device); nothing here needs a GPU.
The error bounds are twice the restatement's own worst case over OTHER seeds (8100 - 8111, motion flag off and on, default
parameters: 2.89 mm and 5.79 degrees over the 168 carried steps), as section 18 set its bounds."""
import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import fit_track_ref as ft
import fit_track_scenes as sc

W, H = 160, 120
POS_BOUND_MM, ROT_BOUND_DEG = 5.8, 11.6          # 2 x (2.89 mm, 5.79 degrees)


@pytest.fixture(scope="module")
def angles(hip_lib):
    from depthhead_amd import fit
    a = fit.angles()
    a.setflags(write=False)
    return a


def tracker(K, angles, flags=0, **prm):
    v, _, nrm = fs.head()
    return ft.Tracker(np.asarray(K)[None], v, nrm, angles, flags=flags, prm=ft.params(**prm))


def run(tr, frames, poses, support=None, present=None):
    out = []
    for k in range(len(frames)):
        sup = sc.good_support() if support is None else support[k:k + 1]
        out.append(tr.step(frames[k][None], poses[k:k + 1], sup, None if present is None else [present[k]])[0])
    return np.array(out)


def kinds(rec):
    return (rec["status"] & 0xFF).tolist()


@pytest.mark.parametrize("motion", [0, ft.MOTION])
@pytest.mark.parametrize("seed", [8000, 8001, 8002, 8003])
def test_fitted_once_then_carried_within_the_bounds(angles, seed, motion):
    frames, K, pos, Rs, poses = sc.sequence(W, H, seed)
    tr = tracker(K, angles, flags=motion)
    rec = run(tr, frames, poses)
    assert kinds(rec) == [ft.FITTED] + [ft.CARRIED] * 7
    assert rec["age"].tolist() == list(range(1, 9)) and not rec["lost"].any()
    assert rec["fit"]["steps"][0] == 20 and (rec["fit"]["steps"][1:] <= 6).all()
    for k in range(1, 8):
        ep = np.linalg.norm(rec["instance"]["t"][k] - pos[k])
        er = fs.geodesic_deg(rec["instance"]["R"][k].reshape(3, 3), Rs[k])
        print(f"seed {seed} motion {motion} step {k}: {ep:.2f} mm {er:.2f} deg")
        assert ep <= POS_BOUND_MM and er <= ROT_BOUND_DEG, (k, ep, er)
    st = tr.state[0]
    assert st["tracked"] == 1 and st["have_prev"] == 1 and st["age"] == 8
    assert st["t"].tobytes() == rec["instance"]["t"][7].tobytes() and st["t_prev"].tobytes() == rec["instance"]["t"][6].tobytes()
    assert st["R"].tobytes() == rec["instance"]["R"][7].tobytes()


@pytest.mark.parametrize("stale_detection", [False, True])
def test_head_gone_for_two_frames_and_back(angles, stale_detection):
    """Frames 3 and 4 are empty.  Frame 3: the carried start finds no point, REJECTED (the fit's status and the point count).
    Frame 4: nothing is tracked; without a valid detection there is no start (NONE), with a stale one its fit is rejected too.
    Frame 5: FITTED again from the forest's pose, then carried."""
    frames, K, pos, Rs, poses = sc.sequence(W, H, 8004, gone=(3, 4))
    sup = sc.good_support(8)
    if not stale_detection:
        sup["mass"][3:5] = 0
    tr = tracker(K, angles)
    rec = run(tr, frames, poses, sup)
    rejected = ft.REJECTED | ft.BAD_STATUS | ft.BAD_POINTS
    assert rec["status"].tolist() == [ft.FITTED, ft.CARRIED, ft.CARRIED, rejected, rejected if stale_detection else ft.NONE, ft.FITTED,
                                      ft.CARRIED, ft.CARRIED]
    assert rec["lost"].tolist() == [0, 0, 0, 1, 2, 0, 0, 0] and rec["age"].tolist() == [1, 2, 3, 0, 0, 1, 2, 3]
    assert rec["fit"]["status"][3] == fr.FEW_POINTS and rec["fit"]["steps"][5] == 20
    assert not np.frombuffer(rec[4]["instance"].tobytes(), np.uint8).any() or stale_detection
    # the rejected record carries its start: the state's instance at frame 3
    assert rec["instance"]["t"][3].tobytes() == rec["instance"]["t"][2].tobytes()
    for k in (5, 6, 7):
        assert np.linalg.norm(rec["instance"]["t"][k] - pos[k]) <= POS_BOUND_MM


def test_absent_cameras_coast_and_are_dropped_beyond_max_coast(angles):
    frames, K, pos, Rs, poses = sc.sequence(W, H, 8005)
    tr = tracker(K, angles, max_coast=2)
    run(tr, frames[:2], poses[:2])
    kept = tr.state[0].copy()
    rec = run(tr, frames[2:4], poses[2:4], present=[0, 0])
    assert kinds(rec) == [ft.ABSENT] * 2 and rec["lost"].tolist() == [1, 2] and rec["age"].tolist() == [2, 2]
    assert not np.frombuffer(rec["instance"].tobytes(), np.uint8).any() and not np.frombuffer(rec["fit"].tobytes(), np.uint8).any()
    st = tr.state[0]
    assert st["tracked"] == 1 and st["have_prev"] == 0 and st["R"].tobytes() == kept["R"].tobytes() and st["t"].tobytes() == kept["t"].tobytes()
    back = run(tr, frames[1:2], poses[1:2])                  # the head where it was left: carried on (no motion start: have_prev was 0)
    assert kinds(back) == [ft.CARRIED] and back["age"][0] == 3 and back["lost"][0] == 0 and tr.state[0]["have_prev"] == 1
    assert tr.state[0]["t_prev"].tobytes() == kept["t"].tobytes()
    tr.reset()
    run(tr, frames[:2], poses[:2])
    rec = run(tr, frames[2:5], poses[2:5], present=[0, 0, 0])
    assert rec["lost"].tolist() == [1, 2, 3] and rec["age"].tolist() == [2, 2, 0]
    assert tr.state[0]["tracked"] == 0 and tr.state[0]["t"].tobytes() == kept["t"].tobytes()
    again = run(tr, frames[5:6], poses[5:6])
    assert again["status"].tolist() == [ft.FITTED] and again["age"][0] == 1 and again["lost"][0] == 0 and tr.state[0]["have_prev"] == 0


def test_motion_flag_extrapolates_in_f32(angles):
    """With no tracked iterations the fit hands its start back: the third step's output is t1 + (t1 - t0) with the flag, t1
    without it, bit for bit."""
    frames, K, pos, Rs, poses = sc.sequence(W, H, 8006)
    got = {}
    for flags in (0, ft.MOTION):
        tr = tracker(K, angles, flags=flags)
        run(tr, frames[:2], poses[:2])
        tr.prm = ft.params(iterations_tracked=0, rms_max=4096.0, keep_points=1)
        t0, t1 = tr.state[0]["t_prev"].copy(), tr.state[0]["t"].copy()
        assert tr.state[0]["have_prev"] == 1
        rec = run(tr, frames[2:3], poses[2:3])
        assert kinds(rec) == [ft.CARRIED] and rec["fit"]["steps"][0] == 0
        got[flags] = rec["instance"]["t"][0]
        want = t1 + (t1 - t0) if flags else t1
        assert got[flags].tobytes() == want.astype(np.float32).tobytes()
    assert got[0].tobytes() != got[ft.MOTION].tobytes()
    # without have_prev (the first carried step) the flag changes nothing
    a, b = tracker(K, angles), tracker(K, angles, flags=ft.MOTION)
    assert run(a, frames[:2], poses[:2]).tobytes() == run(b, frames[:2], poses[:2]).tobytes()


def torso_pose(pos, pose):
    p = pose.copy()
    p["mid_point"] = np.round(pos + (0.0, 300.0, 100.0))          # inside the torso box
    return p.reshape(1)


def test_a_fit_pulled_away_is_rejected_by_max_jump(angles):
    frames, K, pos, Rs, poses = sc.sequence(W, H, 8007)
    tr = tracker(K, angles, rms_max=4096.0, max_jump=60.0)
    rec = run(tr, frames[:1], torso_pose(pos[0], poses[0]))
    assert not tr.state[0]["t"].any() and tr.state[0]["tracked"] == 0 and tr.state[0]["lost"] == 1      # R, t untouched
    assert rec["status"].tolist() == [ft.REJECTED | ft.BAD_JUMP] and rec["fit"]["status"][0] == fr.OK
    assert rec["instance"]["t"][0].tolist() == torso_pose(pos[0], poses[0])["mid_point"][0].tolist()      # the start, not the fit
    # the defaults reject it as well: a head model on a box leaves a large residual
    rec = run(tracker(K, angles), frames[:1], torso_pose(pos[0], poses[0]))
    assert kinds(rec) == [ft.REJECTED] and rec["status"][0] & ft.BAD_RMS
    # a tracked camera is held to the detection too: carried onto the head, the detection on the torso 300 mm away
    tr = tracker(K, angles)
    run(tr, frames[:1], poses[:1])
    rec = run(tr, frames[1:2], torso_pose(pos[1], poses[1]))
    assert rec["status"].tolist() == [ft.REJECTED | ft.BAD_JUMP]
    sup = sc.good_support()
    sup["mass"] = 0                                               # no valid detection: nothing to compare with
    tr = tracker(K, angles)
    run(tr, frames[:1], poses[:1])
    assert kinds(run(tr, frames[1:2], torso_pose(pos[1], poses[1]), sup)) == [ft.CARRIED]


def test_every_reject_reason(angles):
    frames, K, pos, Rs, poses = sc.sequence(W, H, 8007)
    seen = 0
    for prm, frame, want in (({}, np.zeros((H, W), np.uint16), ft.BAD_STATUS | ft.BAD_POINTS),
                             ({"keep_points": 150}, frames[0], ft.BAD_POINTS),
                             ({"rms_max": 0.5}, frames[0], ft.BAD_RMS),
                             ({"max_jump": 60.0}, frames[0], ft.BAD_JUMP),
                             ({"keep_points": 150, "rms_max": 0.5, "max_jump": 60.0}, frames[0], ft.BAD_POINTS | ft.BAD_RMS | ft.BAD_JUMP)):
        rec = run(tracker(K, angles, **prm), frame[None], poses[:1])
        assert rec["status"].tolist() == [ft.REJECTED | want], (prm, hex(rec["status"][0]))
        seen |= want
    assert seen == ft.BAD_STATUS | ft.BAD_POINTS | ft.BAD_RMS | ft.BAD_JUMP
    # the rms limit is exact: sum_r2_fixed <= (int64)(rms_max^2 * 2^20) * points
    rec = run(tracker(K, angles), frames[:1], poses[:1])
    e, n = int(rec["fit"]["sum_r2_fixed"][0]), int(rec["fit"]["points"][0])
    lim = np.sqrt((e // n + 1) / 1048576.0)
    assert kinds(run(tracker(K, angles, rms_max=lim * 1.0001), frames[:1], poses[:1])) == [ft.FITTED]
    assert kinds(run(tracker(K, angles, rms_max=lim * 0.99), frames[:1], poses[:1])) == [ft.REJECTED]


def test_detection_validity_edges(angles):
    prm = ft.params()
    s = sc.good_support()[0]
    assert ft.valid(s, prm)
    for field, v in (("total_mass", 0), ("mass", 19), ("windows", 0)):
        t = s.copy(); t[field] = v
        assert not ft.valid(t, prm), field
    t = s.copy(); t["mass"] = 20                                  # 20 * 50 == 1000 * 1: equality is valid
    assert ft.valid(t, prm)
    big = (2 ** 64 - 1) // 50
    t["mass"], t["total_mass"] = big, big * 50                    # products beyond 64 bits
    assert ft.valid(t, prm)
    t["total_mass"] = big * 50 + 1
    assert not ft.valid(t, prm)
    t["mass"], t["total_mass"] = 0, 5
    assert ft.valid(t, ft.params(conf=(0, 1))) and not ft.valid(t, ft.params(conf=(1, 2 ** 32 - 1)))


def test_every_clamp_of_the_angle_index(angles):
    below = np.nextafter(3.14159, 0.0)
    assert ft.angle_index(-3.14159) == 0 and ft.angle_index(below) == 119 and ft.angle_index(3.14159) == 119
    assert ft.angle_index(-4.0) == 0 and ft.angle_index(-np.inf) == 0 and ft.angle_index(np.nan) == 0
    assert ft.angle_index(np.inf) == 119 and ft.angle_index(1e300) == 119
    assert [ft.angle_index(k * sc.BIN) for k in (-60, -59, -1, 0, 1, 58, 59, 60)] == [0, 1, 59, 60, 61, 118, 119, 119]
    # and through a step: the start's R is the table's entries 0 and 119
    frames, K, pos, Rs, poses = sc.sequence(W, H, 8008, steps=1)
    p = poses[:1].copy()
    p["rotation"][0] = (-3.14159, below, -4.0)
    rec = run(tracker(K, angles, keep_points=10 ** 6), frames, p)          # rejected: the record shows the start
    assert kinds(rec) == [ft.REJECTED]
    (c0, s0), (c1, s1), (c2, s2) = angles[0], angles[119], angles[0]
    Rz = np.array([[c0, s0, 0], [-s0, c0, 0], [0, 0, 1]])
    Ry = np.array([[c1, 0, s1], [0, 1, 0], [-s1, 0, c1]])
    Rx = np.array([[1, 0, 0], [0, c2, -s2], [0, s2, c2]])
    assert np.abs(rec["instance"]["R"][0].reshape(3, 3) - Rx @ Ry @ Rz).max() < 1e-6


def test_forest_rotation_is_euler_to_matrix_on_the_grid(angles):
    from depthhead_amd import render
    for k in ((0, 0, 0), (10, -5, 3), (-20, 13, -7), (59, -60, 30)):
        r = np.array(k) * sc.BIN
        assert np.abs(ft.forest_rotation(r, angles).reshape(3, 3) - render.euler_to_matrix(np.degrees(r))).max() < 2e-7, k


def test_counters_saturate(angles):
    frames, K, pos, Rs, poses = sc.sequence(W, H, 8008, steps=1)
    tr = tracker(K, angles)
    tr.state[0]["lost"] = ft.U32_MAX
    sup = sc.good_support(); sup["mass"] = 0
    assert run(tr, frames, poses[:1], sup)["lost"].tolist() == [ft.U32_MAX]
    assert run(tr, frames, poses[:1], present=[0])["lost"].tolist() == [ft.U32_MAX]
    tr.state[0]["tracked"], tr.state[0]["age"] = 0, 0
    run(tr, frames, poses[:1])
    tr.state[0]["age"] = ft.U32_MAX
    assert run(tr, frames, poses[:1])["age"].tolist() == [ft.U32_MAX]
