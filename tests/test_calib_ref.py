"""The calibration step's restatement (tests/calib_ref.py) held to scenes whose answer is known, on the CPU
alone: a step from the true table stays at the truth, the sums are the single-view fit's where the two must agree, the restated
driver recovers cameras that start 20 mm and 2 degrees off, and the cameras and pairs that take no part leave no trace.  The
bounds are twice the worst case of seeds 0 .. 11 (the tables of section 24); the asserted seeds are 12 and up.  No GPU."""
import numpy as np
import pytest

import calib_ref as cr
import calib_scenes as cs
import fit_ref as fr
import fit_scenes as fs
import view_fit_scenes as vs

# twice the worst of seeds 0 .. 11 ("From the truth": 1.843 mm, 0.2606 degrees, |d| 1.484 mm, |w| 0.2224 degrees)
TRUE_MM, TRUE_DEG, TRUE_D, TRUE_W_DEG = 3.69, 0.522, 2.97, 0.445
# twice the worst of seeds 0 .. 11 ("Recovery": 1.64 mm, 0.419 degrees, rms 2.40 mm)
END_MM, END_DEG, END_RMS = 3.28, 0.838, 4.80


def rms(rec):
    return float(np.sqrt(int(rec["sum_r2_fixed"]) / 1048576.0 / int(rec["points"])))


@pytest.mark.parametrize("seed", [12, 13])
def test_a_step_from_the_true_table_stays_at_the_truth(seed):
    frames, Ks, Vt, ut, pos, Rs = cs.rig(seed, noise=0, holes=0.0)
    v, _, nrm = fs.head()
    rec = cr.calib_step(frames, Ks, Vt, ut, v, nrm, cs.true_instances(pos, Rs), list(range(len(pos))), None, cs.HOLD,
                        cr.params(pivot=pos.mean(axis=0)))
    assert rec["status"].tolist() == [cr.OK, cr.HELD, cr.OK]
    V, u = cr.next_table(Vt, ut, rec)
    err = cs.errors(V, u, Vt, ut, pos)
    print("from the truth, seed", seed, err, rec["delta"].tolist())
    assert err[cs.MIDDLE] == (0.0, 0.0)
    for c in (0, 2):
        assert err[c][0] <= TRUE_DEG and err[c][1] <= TRUE_MM
        assert np.abs(rec["delta"][c, :3]).max() <= TRUE_D and np.degrees(np.abs(rec["delta"][c, 3:]).max()) <= TRUE_W_DEG
        assert rec["pairs"][c] == len(pos) and rec["points"][c] >= 40 * len(pos)


@pytest.mark.parametrize("seed,set_", [(12, 0), (13, 3)])
def test_one_camera_at_the_identity_sums_what_the_fit_sums(seed, set_):
    """V = I, u = 0, the pivot at the instance's t: the translation block, e and count are fit_ref.one_pass's integer for
    integer; the rotation columns are the fit's divided by 64 (exactly, a power of two), so each sum is within the truncation of
    its terms of the fit's sum divided by 64 (mixed block) or 4096 (rotation block)."""
    frames, Ks, Vt, ut, pos, Rs = cs.rig(seed)
    v, _, nrm = fs.head()
    R, t = vs.camera_pose(Vt[cs.MIDDLE], ut[cs.MIDDLE], Rs[set_], pos[set_])
    inst = [{"first_cam": 0, "views": 1, "R": R, "t": t, "scale": np.float32(1.0)}]
    one = frames[set_:set_ + 1, cs.MIDDLE:cs.MIDDLE + 1]
    prm = cr.params(pivot=t.astype(np.float64))
    (A, b, e, count, pairs), = cr.camera_sums(one, Ks[:1], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32), v, nrm, inst, prm=prm)
    fA, fb, fe, fcount = fr.one_pass(one[0, 0], Ks[0], v, nrm, np.float64(1.0), R.astype(np.float64), t.astype(np.float64), prm["gate"])
    assert count == fcount > 40 and e == fe and pairs == 1
    for k, (a_, b_) in enumerate(fr.PAIRS):
        if b_ < 3:
            assert A[k] == fA[k]
        else:
            unit = 64 if a_ < 3 else 4096
            assert abs(A[k] * unit - fA[k]) <= unit * count, (a_, b_)
    assert b[:3] == fb[:3]
    for a_ in range(3, 6):
        assert abs(b[a_] * 64 - fb[a_]) <= 64 * count


@pytest.mark.parametrize("seed", [12, 13, 14, 15])
def test_the_restated_driver_recovers_cameras_20_mm_and_2_degrees_off(seed):
    frames, Ks, Vt, ut, pos, Rs = cs.rig(seed)
    V0, u0 = cs.perturbed(seed)
    v, _, nrm = fs.head()
    start = cs.errors(V0, u0, Vt, ut, pos)
    V, u, inst, trace = cr.calibrate_views(frames, Ks, V0, u0, v, nrm, cs.rough_instances(seed, pos, Rs), list(range(len(pos))), cs.HOLD)
    end = cs.errors(V, u, Vt, ut, pos)
    last = trace[-1]
    print("recovery, seed", seed, "start", start, "end", end, "rms", [rms(r) if r["points"] else None for r in last["records"]])
    # nothing is left out: every instance's last fit is OK and every unheld camera's last record is
    assert [r["status"] for r in last["fit"]] == [fr.OK] * len(pos)
    assert last["records"]["status"].tolist() == [cr.OK, cr.HELD, cr.OK]
    assert len(trace) == 8 + 3 * 2
    assert np.array_equal(V[cs.MIDDLE], V0[cs.MIDDLE]) and np.array_equal(u[cs.MIDDLE], u0[cs.MIDDLE])
    for c in (0, 2):
        assert end[c][0] <= END_DEG and end[c][1] <= END_MM
        assert end[c][0] < start[c][0] / 4.0 and end[c][1] < start[c][1] / 4.0
        assert rms(last["records"][c]) <= END_RMS


def test_cameras_and_pairs_that_take_no_part_leave_no_trace():
    seed = 12
    frames, Ks, Vt, ut, pos, Rs = cs.rig(seed)
    v, _, nrm = fs.head()
    sets = list(range(len(pos)))
    # camera 2 is seen by no instance, camera 1 is held
    inst = cs.true_instances(pos, Rs, views=0b011)
    rec = cr.calib_step(frames, Ks, Vt, ut, v, nrm, inst, sets, None, cs.HOLD)
    assert rec["status"].tolist() == [cr.OK, cr.HELD, cr.FEW_POINTS]
    for c in (1, 2):
        assert rec["V"][c].tobytes() == Vt[c].tobytes() and rec["u"][c].tobytes() == ut[c].tobytes()
        assert rec["points"][c] == 0 and rec["pairs"][c] == 0 and rec["sum_r2_fixed"][c] == 0 and not rec["delta"][c].any()
    # an instance whose pair with camera 0 lies beyond the arm adds nothing to camera 0: the record equals the run without it
    base = cr.calib_step(frames, Ks, Vt, ut, v, nrm, cs.true_instances(pos, Rs), sets, [0, 0, 0, 0, 0, cr.SKIP], cs.HOLD)
    far = cs.true_instances(pos, Rs)
    g = cr.pivot_of(Vt[0].astype(np.float64), ut[0].astype(np.float64), (0.0, 0.0, 0.0))
    far[5]["t"] = (Vt[0].astype(np.float64).T @ (g + np.array([0.0, 0.0, 2050.0]) - ut[0].astype(np.float64))).astype(np.float32)
    got = cr.calib_step(frames, Ks, Vt, ut, v, nrm, far, sets, None, cs.HOLD)
    assert got[0].tobytes() == base[0].tobytes()
    # take = SKIP, a set out of range, no view, a camera out of range and a NaN leave the whole instance out
    for spoil in ({"views": 0}, {"views": 0b1000}, {"first_cam": 2, "views": 0b10}, {"t": np.array([np.nan, 0, 0], np.float32)},
                  {"R": (2.0 * np.eye(3)).astype(np.float32)}, {"scale": np.float32(np.inf)}):
        bad = cs.true_instances(pos, Rs)
        bad[5].update(spoil)
        assert cr.calib_step(frames, Ks, Vt, ut, v, nrm, bad, sets, None, cs.HOLD).tobytes() == base.tobytes(), spoil
    assert cr.calib_step(frames, Ks, Vt, ut, v, nrm, cs.true_instances(pos, Rs), sets[:5] + [6], None, cs.HOLD).tobytes() == base.tobytes()


def test_a_singular_system_and_a_table_at_the_tolerance_edge():
    V = np.eye(3, dtype=np.float32)
    u = np.zeros(3, np.float32)
    # a zero pivot with lambda = 0 is out of reach: the 1e-9 added to every diagonal element keeps a zero row's pivot positive
    zero = cr.solve_camera(V, u, [0] * 21, [0] * 6, 0, 100, 1, False, cr.params(lam=0.0))
    assert zero["status"] == cr.OK and not zero["delta"].any()
    # a negative leading sum (only a wrapped or hand-made row has one) is SINGULAR and keeps the entry
    A = [0] * 21
    A[0] = -(1 << 20)
    sing = cr.solve_camera(V, u, A, [0] * 6, 0, 100, 1, False, cr.params())
    assert sing["status"] == cr.SINGULAR and sing["V"].tobytes() == V.tobytes() and not sing["delta"].any()
    # V = 1.0004 I: (V V^T)[0][0] - 1 = 0.0008 passes; a turn leaves the Gram matrix alone, so the update is OK at the edge and
    # NOT_ORTHONORMAL just beyond it (1.0006 I: 0.0012)
    A = [0] * 21
    for a in range(6):
        A[cr.PAIRS.index((a, a))] = 100 << 20
    b = [0, 0, 0, 0, 0, 10 << 20]
    for s, want in ((1.0004, cr.OK), (1.0006, cr.NOT_ORTHONORMAL)):
        Vs = (s * np.eye(3)).astype(np.float32)
        rec = cr.solve_camera(Vs, u, A, b, 0, 100, 1, False, cr.params())
        assert rec["status"] == want
        if want != cr.OK:
            assert rec["V"].tobytes() == Vs.tobytes() and not rec["delta"].any()
        else:
            assert rec["delta"][5] > 0.001 and rec["V"][1] < 0.0 < rec["V"][3]
