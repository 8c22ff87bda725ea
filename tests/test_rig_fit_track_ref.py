"""The rig fit tracker's rule on the CPU: tests/rig_fit_track_ref.py against the scripts of
tests/rig_fit_track_scenes.py, whose answer is known -- a head moving 5 mm and 2 degrees per step seen by three cameras, the
rig tracker's person records made by hand as the truth plus 60 mm.  The angle table comes from the library
(dh_fit_tracker_angles needs no device); nothing here needs a GPU.  The error bounds are twice the restatement's own worst case
over OTHER seeds (script "carried", seeds 9100 - 9107, motion flag off and on, default parameters: 2.05 mm and 3.67 degrees over
the 112 carried steps), as sections 18 to 21 set theirs."""
import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import rig_fit_track_ref as rf
import rig_fit_track_scenes as sc

POS_BOUND_MM, ROT_BOUND_DEG = 4.1, 7.34          # 2 x (2.05 mm, 3.67 degrees)
NOBODY = rf.NO_PERSON


@pytest.fixture(scope="module")
def angles(hip_lib):
    from depthhead_amd import fit
    a = fit.angles()
    a.setflags(write=False)
    return a


def run(s, angles, steps=None):
    """The script through the restatement: (tracker, records [steps, n_rigs, 16], the state after every step)."""
    v, _, nrm = fs.head()
    tr = rf.Tracker(s["Ks"], s["V"], s["u"], s["rig_begin"], v, nrm, angles, flags=s["flags"], prm=rf.params(**s["prm"]))
    recs, states = [], []
    for st in s["steps"][:steps]:
        fit_prm = fr.params(*st["fit"]) if st["fit"] else None
        recs.append(tr.step(st["frames"], *st["inputs"], present=st["present"], fit_prm=fit_prm))
        states.append(tr.state.copy())
    return tr, np.array(recs), np.array(states)


def zero(a):
    return not np.frombuffer(a.tobytes(), np.uint8).any()


@pytest.mark.parametrize("motion", [0, rf.MOTION])
@pytest.mark.parametrize("seed", [9000, 9001, 9002, 9003])
def test_detected_once_then_carried_within_the_bounds(angles, seed, motion):
    s = sc.script("carried", seed, motion)
    tr, rec, states = run(s, angles)
    r = rec[:, 0, 0]
    assert r["status"].tolist() == [rf.FITTED] + [rf.CARRIED] * 7 and (r["id"] == 7).all() and (r["person"] == 0).all()
    assert r["age"].tolist() == list(range(1, 9)) and not r["lost"].any()
    # a carried step takes fewer passes than a detected one: at most 6 steps and the last pass against 20 and the last pass
    assert r["fit"]["steps"][0] == 20 and (r["fit"]["steps"][1:] <= 6).all()
    assert (r["fit"]["views_used"] == 0b111).all() and (r["instance"]["views"] == 0b111).all() and not r["instance"]["first_cam"].any()
    for k in range(1, 8):
        ep = np.linalg.norm(r["instance"]["t"][k] - s["pos"][k])
        er = fs.geodesic_deg(r["instance"]["R"][k].reshape(3, 3), s["Rs"][k])
        print(f"seed {seed} motion {motion} step {k}: {ep:.2f} mm {er:.2f} deg")
        assert ep <= POS_BOUND_MM and er <= ROT_BOUND_DEG, (k, ep, er)
    assert zero(rec[:, 0, 1:]) and zero(states[:, 0, 1:])
    e = tr.state[0, 0]
    assert (e["id"], e["tracked"], e["have_prev"], e["age"], e["lost"], e["views_used"]) == (7, 1, 1, 8, 0, 0b111)
    assert e["t"].tobytes() == r["instance"]["t"][7].tobytes() and e["t_prev"].tobytes() == r["instance"]["t"][6].tobytes()
    assert e["R"].tobytes() == r["instance"]["R"][7].tobytes()


def test_the_detected_start_is_the_view_table_transposed_times_the_heads_rotation(angles):
    """The start of the first step, read back from a run without iterations: t is the person's world, R the best camera's V^T
    times section 19's rotation of the head's angles, within f32 of the same product in numpy and orthonormal."""
    import fit_track_ref as ft
    s = sc.script("carried", 9001)
    v, _, nrm = fs.head()
    tr = rf.Tracker(s["Ks"], s["V"], s["u"], s["rig_begin"], v, nrm, angles, prm=rf.params(keep_points=0, rms_max=4096.0, max_jump=4096.0))
    for k in (0, 1, 2):
        tr.reset()
        st = s["steps"][k]
        n_heads, heads, n_persons, persons = st["inputs"]
        r = tr.step(st["frames"], *st["inputs"], fit_prm=fr.params(0, 0))[0, 0]
        p = persons[0, 0]
        b = int(p["best_cam"])
        assert b == k and r["fit"]["steps"] == 0 and r["status"] == rf.FITTED
        assert r["instance"]["t"].tobytes() == p["world"].tobytes()
        Rh = ft.forest_rotation(heads[b, 0]["pose"]["rotation"], angles).reshape(3, 3).astype(np.float64)
        want = s["V"][b].astype(np.float64).T @ Rh
        got = r["instance"]["R"].reshape(3, 3).astype(np.float64)
        assert np.abs(got - want).max() < 1e-6 and np.abs(got @ got.T - np.eye(3)).max() < 1e-5
        assert fs.geodesic_deg(got, s["Rs"][k]) < 4.0            # the truth on a 3-degree grid


def test_motion_flag_extrapolates_in_f32(angles):
    """With no tracked iterations the fit hands its start back: the third step's output is t1 + (t1 - t0) with the flag, t1
    without it, bit for bit."""
    got = {}
    for flags in (0, rf.MOTION):
        s = sc.script("carried", 9002, flags)
        tr, _, _ = run(s, angles, steps=2)
        tr.prm = rf.params(iterations_tracked=0, rms_max=4096.0, keep_points=1)
        e = tr.state[0, 0]
        t0, t1 = e["t_prev"].copy(), e["t"].copy()
        assert e["have_prev"] == 1
        st = s["steps"][2]
        r = tr.step(st["frames"], *st["inputs"])[0, 0]
        assert r["status"] == rf.CARRIED and r["fit"]["steps"] == 0
        got[flags] = (r["instance"]["t"].copy(), t0, t1)
    t, t0, t1 = got[rf.MOTION]
    assert t.tobytes() == (t1 + (t1 - t0)).astype(np.float32).tobytes() and t.tobytes() != t1.tobytes()
    assert got[0][0].tobytes() == got[0][2].tobytes()


def test_an_absent_camera_is_left_out_and_an_absent_rig_keeps_its_state(angles):
    s = sc.script("absent", 9003)
    tr, rec, states = run(s, angles)
    r = rec[:, 0, 0]
    assert r["status"].tolist() == [rf.FITTED, rf.CARRIED, rf.CARRIED, rf.CARRIED, rf.ABSENT, rf.ABSENT, rf.CARRIED]
    assert r["instance"]["views"].tolist() == [7, 7, 5, 7, 0, 0, 7] and r["fit"]["views_used"].tolist() == [7, 7, 5, 7, 0, 0, 7]
    assert states[2, 0, 0]["views_used"] == 5 and states[3, 0, 0]["views_used"] == 7
    # the whole rig absent: every record ABSENT and nothing else, the state untouched (no ageing, no coasting)
    for k in (4, 5):
        assert (rec[k, 0]["status"] == rf.ABSENT).all()
        blank = rec[k, 0].copy()
        blank["status"] = 0
        assert zero(blank) and states[k].tobytes() == states[3].tobytes()
    assert r["age"][6] == 5 and states[6, 0, 0]["have_prev"] == 1
    assert np.linalg.norm(r["instance"]["t"][6] - s["pos"][6]) <= POS_BOUND_MM


def test_an_entry_none_of_whose_views_is_present_coasts_and_is_freed_beyond_max_coast(angles):
    s = sc.script("coast", 9000)
    tr, rec, states = run(s, angles)
    r = rec[:, 0, 0]
    assert r["status"].tolist() == [rf.FITTED, rf.CARRIED, rf.ABSENT, rf.ABSENT, rf.ABSENT, rf.FITTED, rf.CARRIED]
    assert r["lost"].tolist() == [0, 0, 1, 2, 3, 0, 0] and r["age"].tolist() == [1, 2, 2, 2, 2, 1, 2]
    assert (r["id"] == 7).all() and r["person"].tolist() == [0, 0, NOBODY, NOBODY, NOBODY, 0, 0]
    assert (r["fit"]["views_used"][:2] == 0b011).all() and zero(r["instance"][2:5]) and zero(r["fit"][2:5])
    kept = states[1, 0, 0]
    for k in (2, 3):
        e = states[k, 0, 0]
        assert (e["id"], e["tracked"], e["have_prev"], e["lost"]) == (7, 1, 0, k - 1) and e["t"].tobytes() == kept["t"].tobytes()
    assert zero(states[4])                                     # lost 3 > max_coast 2: freed
    assert states[5, 0, 0]["id"] == 7 and states[5, 0, 0]["have_prev"] == 0 and r["fit"]["steps"][5] == 20


def test_an_empty_frame_rejects_keeps_the_id_and_the_next_step_starts_from_the_detection(angles):
    s = sc.script("gone", 9001)
    tr, rec, states = run(s, angles)
    r = rec[:, 0, 0]
    rejected = rf.REJECTED | rf.BAD_STATUS | rf.BAD_POINTS
    assert r["status"].tolist() == [rf.FITTED, rf.CARRIED, rf.CARRIED, rejected, rf.FITTED, rf.CARRIED]
    assert r["lost"].tolist() == [0, 0, 0, 1, 0, 0] and r["age"].tolist() == [1, 2, 3, 0, 1, 2] and (r["id"] == 7).all()
    assert r["fit"]["status"][3] == fr.FEW_POINTS and r["fit"]["steps"][4] == 20 and r["fit"]["steps"][3] == 0
    # the rejected record carries its start, the state's pose; the entry stays bound, untracked
    assert r["instance"]["t"][3].tobytes() == r["instance"]["t"][2].tobytes()
    e = states[3, 0, 0]
    assert (e["id"], e["tracked"], e["have_prev"], e["age"], e["lost"]) == (7, 0, 0, 0, 1)
    assert r["instance"]["t"][4].tobytes() != r["instance"]["t"][2].tobytes() and states[4, 0, 0]["have_prev"] == 0
    for k in (4, 5):
        assert np.linalg.norm(r["instance"]["t"][k] - s["pos"][k]) <= POS_BOUND_MM


def test_an_unseen_person_is_followed_by_the_model_and_freed_when_it_is_rejected(angles):
    s = sc.script("unseen", 9002)
    tr, rec, states = run(s, angles)
    r = rec[:, 0, 0]
    rejected = rf.REJECTED | rf.BAD_STATUS | rf.BAD_POINTS
    assert r["status"].tolist() == [rf.FITTED, rf.CARRIED, rf.CARRIED, rf.CARRIED, rejected, rf.FITTED]
    assert r["person"].tolist() == [0, 0, NOBODY, NOBODY, NOBODY, 0] and (r["id"] == 7).all()
    assert r["age"].tolist() == [1, 2, 3, 4, 0, 1] and r["lost"].tolist() == [0, 0, 0, 0, 1, 0]
    for k in (2, 3):                                           # no detection, and still on the head
        assert np.linalg.norm(r["instance"]["t"][k] - s["pos"][k]) <= POS_BOUND_MM
        assert states[k, 0, 0]["lost"] == 0 and states[k, 0, 0]["age"] == k + 1
    assert zero(states[4])                                     # rejected and unseen: freed
    assert states[5, 0, 0]["id"] == 7 and states[5, 0, 0]["age"] == 1


def test_a_person_record_200_mm_off_is_a_bad_jump(angles):
    s = sc.script("jump", 9003)
    tr, rec, states = run(s, angles)
    r = rec[:, 0, 0]
    assert r["status"].tolist() == [rf.FITTED, rf.CARRIED, rf.REJECTED | rf.BAD_JUMP, rf.FITTED, rf.CARRIED, rf.CARRIED]
    world = s["steps"][2]["inputs"][3][0, 0]["world"]
    assert 190.0 < np.linalg.norm(world - s["pos"][2]) < 210.0
    # the fit itself was good: it is the detection that is not believed against it -- or the other way round
    assert r["fit"]["status"][2] == fr.OK and r["fit"]["points"][2] >= 30
    assert states[2, 0, 0]["id"] == 7 and states[2, 0, 0]["tracked"] == 0 and r["instance"]["t"][2].tobytes() == r["instance"]["t"][1].tobytes()


def test_id_0_a_repeated_id_and_a_person_that_names_no_head(angles):
    s = sc.script("unbound", 9000)
    tr, rec, states = run(s, angles)
    # step 0: person 1 founds entry 0 with id 5; persons 0 (id 0) and 2 (id 5 again) take the record slots 1 and 2
    r = rec[0, 0]
    assert r["id"][:4].tolist() == [5, 0, 5, 0] and r["person"][:3].tolist() == [1, 0, 2] and r["status"][:4].tolist() == [rf.FITTED] * 3 + [0]
    assert r["age"][:3].tolist() == [1, 1, 1] and zero(r[3:])
    assert states[0, 0, 0]["id"] == 5 and states[0, 0, 0]["tracked"] == 1 and zero(states[0, 0, 1:])
    # step 1: person 0 names no head and is ignored; person 2 is still unbound and now first in line
    r = rec[1, 0]
    assert r["id"][:3].tolist() == [5, 5, 0] and r["person"][:2].tolist() == [1, 2] and r["status"][:3].tolist() == [rf.CARRIED, rf.FITTED, 0]
    assert zero(r[2:]) and zero(states[1, 0, 1:])
    # step 2: as step 0; an unbound person is never carried
    r = rec[2, 0]
    assert r["status"][:3].tolist() == [rf.CARRIED, rf.FITTED, rf.FITTED] and r["fit"]["steps"][1] == 20 and r["age"][:3].tolist() == [3, 1, 1]


@pytest.mark.parametrize("motion", [0, rf.MOTION])
def test_two_rigs_the_second_beginning_at_camera_1(angles, motion):
    s = sc.script("two_rigs", 9001, motion)
    tr, rec, states = run(s, angles)
    r = rec[:, 1, 0]
    assert r["status"].tolist() == [rf.FITTED, rf.CARRIED, rf.CARRIED, rf.CARRIED, rf.ABSENT, rf.CARRIED]
    assert (r["instance"]["first_cam"][[0, 1, 2, 3, 5]] == 1).all() and (r["instance"]["views"][[0, 1, 2, 3, 5]] == 0b111).all()
    assert (rec[3, 0]["status"] == rf.ABSENT).all() and zero(rec[[0, 1, 2, 4, 5], 0]) and zero(states[:, 0])
    assert (rec[4, 1]["status"] == rf.ABSENT).all() and states[4].tobytes() == states[3].tobytes()
    for k in (1, 2, 3, 5):
        assert np.linalg.norm(r["instance"]["t"][k] - s["pos"][k]) <= POS_BOUND_MM
        assert fs.geodesic_deg(r["instance"]["R"][k].reshape(3, 3), s["Rs"][k]) <= ROT_BOUND_DEG


def test_a_seventeenth_id_finds_no_entry_and_is_reported_without_being_carried(angles):
    s = sc.script("full", 9002)
    tr, rec, states = run(s, angles)
    r = rec[0, 0]
    assert r["id"].tolist() == list(range(1, 17)) and r["person"].tolist() == list(range(16))
    assert (r["status"][:15] == rf.FITTED).all() and (r["status"][15] & 0xFF) == rf.REJECTED     # (200 mm off, one view, 4 steps)
    assert states[0, 0]["id"].tolist() == list(range(1, 17)) and states[0, 0]["tracked"].tolist() == [1] * 15 + [0]
    # id 17 finds every entry taken; the entry of id 16 (unseen, not tracked) is freed after the walk and its record slot
    # reports person 0; id 3 is seen; the others are followed unseen
    r = rec[1, 0]
    assert r["id"].tolist() == list(range(1, 16)) + [17] and r["person"].tolist() == [NOBODY, NOBODY, 1] + [NOBODY] * 12 + [0]
    assert (r["status"][:15] & 0xFF != rf.FITTED).all() and r["status"][15] == rf.FITTED and r["age"][15] == 1
    assert states[1, 0, 15]["id"] == 0 and zero(states[1, 0, 15])
    # id 18 takes the freed entry
    r = rec[2, 0]
    assert r["id"][15] == 18 and r["person"][15] == 0 and states[2, 0, 15]["id"] == 18
