"""The identification rule as tests/ident_ref.py restates it, on scenes whose answer is known: ties and
the ratio test, the enrolment mask, an empty frame, an instance whose fit failed, iterations = 0 against one pass of the fit,
the answer handed to a surface step, and the evaluation -- three enrolled subjects, held-out probes of each and of a stranger --
under the shipped defaults.  Run as a program it prints the evaluation's table.  No GPU."""
import numpy as np

import fit_ref as fr
import ident_ref as ir
import ident_scenes as isc
import surface_ref as su

W, H = 96, 96


def small(truth=(0, 1, 2, 1), n_subjects=3, **kw):
    return isc.gallery("642", n_subjects, W, H, list(truth), **kw)


def test_the_true_subject_wins_and_the_outputs_agree_with_the_scores():
    _, _, _, frames, K, inst, st = small()
    subjects, rec, poses, scores = ir.identify(frames, K, st, inst, prm=ir.params(max_rms=np.inf))
    assert subjects.tolist() == [0, 1, 2, 1] and (rec["status"] == ir.OK).all() and (rec["eligible"] == 3).all()
    for i in range(4):
        m = [float(ir.mean_square(s["sum_r2_fixed"], s["points"])) for s in scores[i]]
        order = sorted(range(3), key=lambda s: (m[s], s))
        assert (rec["best"][i], rec["second"][i]) == (order[0], order[1])
        assert (rec["points_best"][i], rec["sum_r2_best"][i]) == (scores[i, order[0]]["points"], scores[i, order[0]]["sum_r2_fixed"])
        assert (rec["points_second"][i], rec["sum_r2_second"][i]) == (scores[i, order[1]]["points"], scores[i, order[1]]["sum_r2_fixed"])
        R, t, _ = ir.score(frames[i], K, st.pts[order[0]], st.nrm[order[0]], inst[i], ir.params())
        assert poses[i]["R"].tobytes() == R.tobytes() and poses[i]["t"].tobytes() == t.tobytes() and poses[i]["frame"] == i


def test_one_subject_twice_gives_the_lower_index_and_the_ratio_test_calls_it_ambiguous():
    _, _, _, frames, K, inst, st = small(truth=(1, 1), n_subjects=3)
    st.set_coeffs(np.array([[0.1], [0.1], [-0.4]]))                                 # subjects 0 and 1 identical
    _, _, _, frames, K, inst, _ = isc.gallery("642", 3, W, H, [1, 1])
    for ratio, status, out in ((1.0, ir.OK, 0), (1.5, ir.AMBIGUOUS, ir.UNKNOWN)):
        subjects, rec, _, scores = ir.identify(frames, K, st, inst, prm=ir.params(max_rms=np.inf, min_ratio=ratio))
        assert scores[:, 0].tobytes() == scores[:, 1].tobytes()
        assert (rec["status"] == status).all() and (rec["best"] == 0).all() and (rec["second"] == 1).all() and (subjects == out).all()
    # one candidate: no second, and the ratio test cannot apply
    subjects, rec, _, _ = ir.identify(frames, K, st, inst, n_subjects=1, prm=ir.params(max_rms=np.inf, min_ratio=100.0))
    assert (rec["status"] == ir.OK).all() and (rec["second"] == ir.UNKNOWN).all() and (rec["eligible"] == 1).all() and (subjects == 0).all()


def test_an_unenrolled_better_match_is_never_chosen():
    _, _, _, frames, K, inst, st = small()
    subjects, rec, _, scores = ir.identify(frames, K, st, inst, enrolled=[1, 0, 1], prm=ir.params(max_rms=np.inf))
    assert 1 not in subjects.tolist() and 1 not in rec["best"].tolist() and 1 not in rec["second"].tolist()
    assert not scores[:, 1].tobytes().strip(b"\0") and (rec["eligible"] == 2).all()
    assert subjects[0] == 0 and subjects[2] == 2
    subjects, rec, poses, scores = ir.identify(frames, K, st, inst, enrolled=[0, 0, 0])
    assert (rec["status"] == ir.NO_CANDIDATE).all() and (subjects == ir.UNKNOWN).all() and not scores.tobytes().strip(b"\0")
    assert all(p["t"].tobytes() == i["t"].tobytes() for p, i in zip(poses, inst))


def test_an_empty_frame_a_failed_fit_and_the_limit():
    _, _, _, frames, K, inst, st = small()
    frames = frames.copy()
    frames[0] = 0
    status = [fr.OK, fr.FEW_POINTS, fr.OK, fr.SINGULAR]
    subjects, rec, poses, scores = ir.identify(frames, K, st, inst, fit_status=status, prm=ir.params(max_rms=np.inf))
    assert rec["status"].tolist() == [ir.NO_CANDIDATE, ir.SKIPPED, ir.OK, ir.SKIPPED] and subjects.tolist() == [ir.UNKNOWN, ir.UNKNOWN, 2, ir.UNKNOWN]
    assert (scores[0]["status"] == fr.FEW_POINTS).all() and (scores[0]["points"] == 0).all() and rec["eligible"][0] == 0
    for i in (0, 1, 3):                                                             # the pose copied through
        assert poses[i]["R"].tobytes() == inst[i]["R"].tobytes() and poses[i]["t"].tobytes() == inst[i]["t"].tobytes()
        assert (rec["best"][i], rec["second"][i]) == (ir.UNKNOWN, ir.UNKNOWN)
    assert not scores[1].tobytes().strip(b"\0") and not scores[3].tobytes().strip(b"\0")
    # both sides of the limit: max_rms^2 just above and just below the best mean square
    m = float(ir.mean_square(rec["sum_r2_best"][2], rec["points_best"][2]))
    above, below = np.sqrt(m) * (1 + 1e-9), np.sqrt(m) * (1 - 1e-9)
    assert above * above >= m > below * below
    assert ir.identify(frames, K, st, inst[2:3], prm=ir.params(max_rms=above))[1]["status"][0] == ir.OK
    far = ir.identify(frames, K, st, inst[2:3], prm=ir.params(max_rms=below))
    assert far[1]["status"][0] == ir.FAR and far[0][0] == ir.UNKNOWN and far[1]["best"][0] == 2
    assert far[2][0]["t"].tobytes() != inst[2]["t"].tobytes()                       # E is not empty: the refitted pose


def test_no_iterations_is_one_pass_of_the_fit():
    _, _, _, frames, K, inst, st = small()
    _, rec, poses, scores = ir.identify(frames, K, st, inst, prm=ir.params(iterations=0, max_rms=np.inf))
    for i, it in enumerate(inst):
        for s in range(3):
            _, _, e, count = fr.one_pass(frames[i], np.asarray(K, np.float32).reshape(3, 3).astype(np.float64), st.pts[s], st.nrm[s],
                                         np.float64(it["scale"]), it["R"].astype(np.float64), it["t"].astype(np.float64), 25.0)
            assert (scores[i, s]["points"], scores[i, s]["sum_r2_fixed"], scores[i, s]["steps"], scores[i, s]["status"]) == (count, e, 0, fr.OK)
        assert poses[i]["t"].tobytes() == it["t"].tobytes() and poses[i]["R"].tobytes() == it["R"].tobytes()


def test_the_answer_handed_to_a_surface_step_skips_exactly_the_unknown_instances():
    _, _, _, frames, K, inst, st = small(truth=(0, 1, 2, 1, 0, 2), surface=True)
    frames = frames.copy()
    frames[3] = 0                                                                   # an unknown head
    subjects, rec, poses, _ = ir.identify(frames, K, st, inst, prm=ir.params(max_rms=np.inf))
    assert subjects.tolist() == [0, 1, 2, ir.UNKNOWN, 0, 2]
    srec = su.surface_step(frames, K, st, poses, subjects, 3, None, su.params(min_points=1))
    assert srec["instances"].tolist() == [2, 1, 2]
    known = [i for i in range(6) if subjects[i] != ir.UNKNOWN]
    st2 = isc.gallery("642", 3, W, H, [0, 1, 2, 1, 0, 2], surface=True)[6]
    alone = su.surface_step(frames, K, st2, [poses[i] for i in known], subjects[known], 3, None, su.params(min_points=1))
    assert alone.tobytes() == srec.tobytes() and st2.offsets.tobytes() == st.offsets.tobytes()


def evaluation_table():
    """(rows of (probe, truth, status, best, second, best mean square, second / best), largest known, smallest stranger)."""
    _, _, _, _, _, truth = isc.evaluation()
    subjects, rec, _, _ = isc.evaluation_result()
    rows = []
    for i, who in enumerate(truth):
        mb = float(ir.mean_square(rec["sum_r2_best"][i], rec["points_best"][i]))
        ms = float(ir.mean_square(rec["sum_r2_second"][i], rec["points_second"][i]))
        rows.append((i, who, int(rec["status"][i]), int(rec["best"][i]), int(rec["second"][i]), mb, ms / mb, int(subjects[i])))
    return rows, max(r[5] for r in rows if r[1] is not None), min(r[5] for r in rows if r[1] is None)


def test_the_evaluation_under_the_shipped_defaults():
    """All 12 known probes DH_IDENT_OK with the right subject, all 4 stranger probes DH_IDENT_FAR.  Measured with this file:
    largest best mean square of a known probe 2.2557 mm^2, smallest of a stranger probe 3.5547 mm^2: the default max_rms is
    sqrt(sqrt(2.2557 * 3.5547)) = 1.6828, shipped as 1.68."""
    rows, known, stranger = evaluation_table()
    for i, who, status, best, second, mb, ratio, out in rows:
        print(i, who, status, best, second, round(mb, 4), round(ratio, 3))
        if who is None:
            assert (status, out) == (ir.FAR, ir.UNKNOWN), rows[i]
        else:
            assert (status, best, out) == (ir.OK, who, who), rows[i]
    assert known < ir.DEFAULT_MAX_RMS ** 2 < stranger
    assert abs(np.sqrt(np.sqrt(known * stranger)) - ir.DEFAULT_MAX_RMS) < 0.01, (known, stranger)   # the default is the measured midpoint


if __name__ == "__main__":
    rows, known, stranger = evaluation_table()
    names = {ir.OK: "OK", ir.SKIPPED: "SKIPPED", ir.NO_CANDIDATE: "NO_CANDIDATE", ir.FAR: "FAR", ir.AMBIGUOUS: "AMBIGUOUS"}
    print("probe truth    status best second  m_best mm^2  second/best")
    for i, who, status, best, second, mb, ratio, _ in rows:
        print(f"{i:5d} {'stranger' if who is None else who!s:8} {names[status]:6} {best:4d} {second:6d} {mb:12.4f} {ratio:12.3f}")
    print(f"largest known {known:.4f} mm^2, smallest stranger {stranger:.4f} mm^2, sqrt of the geometric mean {np.sqrt(np.sqrt(known * stranger)):.4f} mm")
