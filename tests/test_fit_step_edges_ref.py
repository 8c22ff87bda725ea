"""The placed cases of tests/fit_step_edges.py on the CPU.  The restatements of the step rule (fit_ref,
view_fit_ref) and of the trackers' rule (fit_track_ref, rig_fit_track_ref) must give the hand-worked literals, at every model
size; the expressions the literals lean on are asserted as written; and the table is proved TIGHT: in local copies of both
rules every compare is relaxed on its own (`>` to `>=`, `<` to `<=`, `<=` to `<`, a test dropped, a clamp moved), and the rows
whose answer changes must be exactly those that fit_step_edges.STEP_FLIPS / TRACK_FLIPS name -- at least one per compare, and no
row under a compare it does not name."""
import functools

import numpy as np
import pytest

import calib_ref as cr
import fit_edges as fe
import fit_ref as fr
import fit_step_edges as se
import fit_track_ref as tkr
import rig_fit_track_ref as rf
import shape_ref as sr
import view_fit_ref as vr

F64 = np.float64
EYE = np.eye(3, dtype=np.float32)
ANGLE_TABLE = np.array([[np.cos((i - 60) / 60.0 * 3.14159), np.sin((i - 60) / 60.0 * 3.14159)] for i in range(120)], F64)
# (any table serves the restatements here: the rows turn on WHICH entry is picked)
PERSON = np.dtype([("views", "<u8"), ("mass", "<u8"), ("cell", "<i4", (3,)), ("n_views", "<u4"), ("world", "<f4", (3,)), ("id", "<u4"),
                   ("best_cam", "<u4"), ("best_head", "<u4")], align=True)
POSE = np.dtype([("mid_point", "<f4", (3,)), ("reserved", "<u4"), ("rotation", "<f8", (3,))], align=True)
SUPPORT = fe.tracker_inputs()[1].dtype
HEAD = np.dtype([("pose", POSE), ("support", SUPPORT)], align=True)


def ref_params(c):
    return fr.params(c.coarse, c.full, c.gate, c.lam, c.min_points)


# ---------------------------------------------------------------- the expressions the literals lean on
def test_the_expressions_of_the_literals():
    res2 = [int((-pz * (F64(8195.0) / pz - 1.0)) ** 2 * 2 ** 20) for pz in (F64(8192.0), F64(8256.0), F64(8320.0))]
    assert res2 == [9 * se.M20, 61 * 61 * se.M20 - 1, 125 * 125 * se.M20 - 1] and se.ZERO_E == 2 * sum(res2)
    a33 = F64(6 * 2 ** 22)
    assert a33 * 1.0 + 1e-9 == a33 and a33 / a33 == 1.0 and a33 - 1.0 * a33 == 0.0
    assert a33 * (1.0 + 2.0 ** -52) + 1e-9 > a33
    for lam, on in ((se.LAM_BELOW, False), (se.LAM_ON, True)):
        x2 = F64(6.0) / (F64(6.0) * (F64(1.0) + F64(lam)) + 1e-9)
        assert (x2 == 1e-6) == on and (x2 < 1e-6) != on
    assert se.LAM_ON < se.LAM_BELOW == np.nextafter(se.LAM_ON, np.inf)
    assert int((1.0 - 1e-6) ** 2 * 2 ** 20) == 1048573 and int((1.0 - 2e-6) ** 2 * 2 ** 20) == 1048571
    for m, positive in ((81, True), (82, False)):
        a23 = F64(m) * 2.0 ** -20
        fourth = (F64(0.0) * 1.0 + 1e-9) - (a23 / (F64(6.0) * 1.0 + 1e-9)) * a23
        third = (F64(6.0) * 1.0 + 1e-9) - (a23 / F64(1e-9)) * a23
        assert (fourth > 0.0) == positive and (third > 0.0) == positive and (not positive or 5.4e-12 < fourth < 5.5e-12)
    for r in se.RMS:
        lim = int(F64(r.rms_max) * F64(r.rms_max) * F64(1048576.0))
        below = F64(np.nextafter(r.rms_max, 0.0))
        assert lim * r.points == r.e and int(below * below * F64(1048576.0)) == lim - 1
    assert np.float32(se.JUMP_BEYOND[2]) == np.nextafter(np.float32(64.0), np.float32(65.0))
    d = F64(se.JUMP_BEYOND[2]) - 64.0
    assert (F64(9.0) + 16.0) + d * d > 25.0 == se.MAX_JUMP * se.MAX_JUMP


# ---------------------------------------------------------------- local copies of the step's pivots and of the lambda search
def pivots(case, n, gate):
    pts, nrm = se.step_model(case, 0)
    A, _, _, _ = fr.one_pass(case.frame, fe.K, pts, nrm, F64(1.0), np.eye(3), np.array(case.t, F64), gate)
    M = [[F64(0.0)] * 6 for _ in range(6)]
    for (a, c), v in zip(fr.PAIRS, A):
        M[a][c] = M[c][a] = F64(v) / fr.S
    for a in range(6):
        M[a][a] = M[a][a] * (F64(1.0) + F64(case.lam)) + 1e-9
    out = []
    with np.errstate(all="ignore"):
        for k in range(n):
            out.append(float(M[k][k]))
            for i in range(k + 1, n):
                f = M[i][k] / M[k][k]
                for j in range(k + 1, n):
                    M[i][j] = M[i][j] - f * M[k][j]
    return out


def test_the_pivots_are_where_the_rows_say():
    z = pivots(se.STEP_BY_NAME["zero_pivot"], 6, 256.0)
    assert z[:4] == [1e-9, 1e-9, 6.0 + 1e-9, float(6 * 2 ** 22)] and z[4] == 0.0
    assert 0.0 < pivots(se.STEP_BY_NAME["zero_pivot_damped"], 6, 256.0)[4] < 1e-7
    z = pivots(se.STEP_BY_NAME["last_pivot_zero"], 6, 256.0)
    assert z[:5] == [6.0 + 1e-9, 1e-9, 1e-9, 1e-9, float(6 * 2 ** 22)] and z[5] == 0.0
    assert 0.0 < pivots(se.STEP_BY_NAME["last_pivot_zero_damped"], 6, 256.0)[5] < 1e-7
    t, n = pivots(se.STEP_BY_NAME["tiny_pivot"], 6, 25.0), pivots(se.STEP_BY_NAME["negative_pivot"], 6, 25.0)
    assert 5.4e-12 < t[3] < 5.5e-12 and all(p > 0.0 for p in t) and -2e-11 < n[3] < 0.0 and all(p > 0.0 for p in n[:3])
    t, n = pivots(se.STEP_BY_NAME["coarse_positive_pivot"], 3, 25.0), pivots(se.STEP_BY_NAME["coarse_negative_pivot"], 3, 25.0)
    assert t[:2] == [1e-9, 1e-9] and 0.03 < t[2] < 0.04 and n[:2] == [1e-9, 1e-9] and -0.2 < n[2] < 0.0


@functools.lru_cache(maxsize=None)
def searched_lambda():
    """The ON row of the early exit found by walking lambda down from 999999.0 in the restatement, once per module: the first
    lambda at which the phase takes a second step, for the coarse and for the full solve.  -> {phase: (lambda, steps walked)}"""
    out = {}
    for phase, name in (("coarse", "coarse_exit_below"), ("full", "full_exit_below")):
        c = se.STEP_BY_NAME[name]
        pts, nrm = se.step_model(c, 0)
        lam = F64(se.LAM_BELOW)
        for walked in range(400):
            rec = fr.fit(c.frame, fe.K, pts, nrm, EYE, c.t, 1.0, fr.params(c.coarse, c.full, c.gate, float(lam), 6))[2]
            if rec["steps"] == 2:
                out[phase] = (float(lam), walked)
                break
            lam = np.nextafter(lam, 0.0)
    return out


def test_the_searched_lambda_is_the_literal():
    assert searched_lambda() == {"coarse": (se.LAM_ON, 1), "full": (se.LAM_ON, 1)}


# ---------------------------------------------------------------- the restatements of the step rule give the literals
def hold(case, R, t, rec, what):
    assert (rec["status"], rec["steps"]) == (case.status, case.steps), (what, case.name, rec)
    if case.points is not None:
        assert rec["points"] == case.points, (what, case.name, rec)
    if case.e is not None:
        assert rec["sum_r2_fixed"] == case.e, (what, case.name, rec)
    assert (R == EYE).all(), (what, case.name)          # no placed case turns the pose: x3 = x4 = x5 = 0 in every step taken
    if case.still:
        assert tuple(t) == case.t, (what, case.name, t)


@pytest.mark.parametrize("n", se.SIZES)
@pytest.mark.parametrize("case", se.STEPS, ids=lambda c: c.name)
def test_the_restatements_give_the_step_literals(case, n):
    pts, nrm = se.step_model(case, n)
    R, t, rec = fr.fit(case.frame, fe.K, pts, nrm, EYE, case.t, 1.0, ref_params(case))
    hold(case, R, t, rec, "fit_ref")
    frames = np.stack([case.frame, np.zeros_like(case.frame)])
    Ks, V, u = np.stack([fe.K, fe.K]), np.stack([EYE, EYE]), np.zeros((2, 3), np.float32)
    for views in (0b01, 0b11):                      # the second view sees an empty frame and adds nothing
        Rv, tv, rv = vr.fit(frames, Ks, V, u, 0, views, pts, nrm, EYE, case.t, 1.0, ref_params(case))
        hold(case, Rv, tv, rv, "view_fit_ref")
        assert Rv.tobytes() == R.tobytes() and tv.tobytes() == t.tobytes() and rv["views_used"] == (1 if rv["points"] else 0)
        assert {k: rv[k] for k in rec} == rec


# ---------------------------------------------------------------- the step rule, every compare relaxed on its own
def local_solve(M, b, n, lam1, relax=None):
    """fit_solve_tri on the leading n x n block of the sums M (damped here) with the pivot compare relaxed or not; None: refused."""
    M = [[F64(v) for v in row] for row in M]
    for a in range(len(M)):
        M[a][a] = M[a][a] * lam1 + 1e-9
    b = list(b)
    ok = True
    with np.errstate(all="ignore"):
        for k in range(n):
            piv = M[k][k]
            ok = ok and bool(piv >= 0.0 if relax == "piv > 0.0 -> >=" else piv > 0.0)
            for i in range(k + 1, n):
                f = M[i][k] / piv
                for j in range(k + 1, n):
                    M[i][j] = M[i][j] - f * M[k][j]
                b[i] = b[i] - f * b[k]
        if not ok:
            return None
        x = [F64(0.0)] * len(M)
        for i in range(n - 1, -1, -1):
            s = b[i]
            for j in range(i + 1, n):
                s = s - M[i][j] * x[j]
            x[i] = s / M[i][i]
    return x


def step_rule(case, relax=None):
    """A local copy of the step rule on fit_ref's pass, solve arithmetic and Cayley update, with one compare relaxed.
    -> (status, steps, R bytes, t bytes)"""
    pts, nrm = se.step_model(case, 0)
    R, t = np.eye(3, dtype=F64), np.array(case.t, F64)
    lam1 = F64(1.0) + F64(case.lam)
    steps, status, stop = 0, se.OK, False

    def solve(A, b, n):
        M = [[F64(0.0)] * 6 for _ in range(6)]
        for (a, c), v in zip(fr.PAIRS, A):
            M[a][c] = M[c][a] = F64(v) / fr.S
        return local_solve(M, [F64(v) / fr.S for v in b], n, lam1, relax)

    def few(count):
        return count <= case.min_points if relax == "count < min_points -> <=" else count < case.min_points

    def small(x, n):
        return all((abs(v) <= 1e-6 if relax == "abs(x) < 1e-6 -> <=" else abs(v) < 1e-6) for v in x[:n])

    with np.errstate(all="ignore"):
        for _ in range(case.coarse):
            A, b, _, count = fr.one_pass(case.frame, fe.K, pts, nrm, F64(1.0), R, t, case.gate[0])
            if few(count):
                status, stop = se.FEW_POINTS, relax != "coarse FEW_POINTS stop dropped"
                break
            x = solve(A, b, 3)
            if x is None:
                status, stop = se.SINGULAR, relax != "coarse SINGULAR stop dropped"
                break
            t = t + np.array(x[:3])
            steps += 1
            if small(x, 3):
                break
        for _ in range(case.full):
            if stop:
                break
            A, b, _, count = fr.one_pass(case.frame, fe.K, pts, nrm, F64(1.0), R, t, case.gate[1])
            if few(count):
                status = se.FEW_POINTS
                break
            x = solve(A, b, 6)
            if x is None:
                status = se.SINGULAR
                break
            t = t + np.array(x[:3])
            R = fr.cayley(R, x[3:6])
            steps += 1
            if small(x, 6):
                break
    return status, steps, R.astype(np.float32).tobytes(), t.astype(np.float32).tobytes()


@functools.lru_cache(maxsize=None)
def step_answers(relax):
    return {c.name: step_rule(c, relax) for c in se.STEPS}


def test_the_local_step_rule_is_the_restated_one():
    for c in se.STEPS:
        R, t, rec = fr.fit(c.frame, fe.K, *se.step_model(c, 0), EYE, c.t, 1.0, ref_params(c))
        assert step_answers(None)[c.name] == (rec["status"], rec["steps"], R.tobytes(), t.tobytes()), c.name


@pytest.mark.parametrize("relax", sorted(se.STEP_FLIPS))
def test_each_relaxed_step_compare_flips_exactly_the_rows_that_name_it(relax):
    plain, relaxed = step_answers(None), step_answers(relax)
    flipped = {name for name in plain if plain[name] != relaxed[name]}
    assert flipped == se.STEP_FLIPS[relax] and flipped, (relax, flipped)


# ---------------------------------------------------------------- the restatements of the trackers' rule give the literals
def frames_of(script, step, cams=1):
    tb = se.tracker_table(script.only)
    frame = np.zeros_like(tb.frames[0]) if step["empty"] else tb.frames[0]
    out = np.zeros((script.n, cams) + frame.shape, np.uint16)
    out[:, 0] = frame
    return tb, out.reshape((script.n * cams,) + frame.shape)


def hold_track(script, step, status, fit, R, tracked, what):
    """One step's records against the literals: the status of every row; points and e wherever a fit ran; the start R of a
    rejected detection against the angle table's entry (the angle rows)."""
    for i, want in enumerate(step["want"]):
        assert status[i] == want, (what, script.name, i, hex(status[i]), hex(want))
        if want not in (se.NONE, se.ABSENT) and step["points"] is not None:
            assert (fit["points"][i], fit["sum_r2_fixed"][i], fit["steps"][i], fit["status"][i]) == (step["points"], step["e"], 0, se.OK), (what, script.name, i)
        if step["tracked"] is not None:
            assert tracked[i] == step["tracked"][i], (what, script.name, i)
    if script.name == "angles":
        for i, (name, rotation, index) in enumerate(se.ANGLES):
            assert tkr.angle_index(rotation) == index, name
            want = tkr.forest_rotation([ANGLE_TABLE_INDEX[index]] * 3, ANGLE_TABLE)
            assert R[i].tobytes() == want.tobytes(), (what, name)


ANGLE_TABLE_INDEX = [(i - 60 + 0.25) * se.BIN for i in range(120)]       # a rotation in the middle of entry i's bin


@pytest.mark.parametrize("script", se.scripts(), ids=lambda s: s.name)
def test_fit_track_ref_gives_the_tracker_literals(script):
    tb = None
    ref = None
    for step in script.steps:
        tb, frames = frames_of(script, step)
        if ref is None:
            kw = dict(script.prm)
            ref = tkr.Tracker(np.stack([fe.K] * script.n), *tb.models[0], ANGLE_TABLE, prm=tkr.params(**kw))
        rec = ref.step(frames, se.poses_of(step, POSE), se.support_of(step["support"]), present=step["present"], fit_prm=fr.params(0, 0, (se.GATE, se.GATE)))
        hold_track(script, step, rec["status"], rec["fit"], rec["instance"]["R"], ref.state["tracked"], "fit_track_ref")
        for i, want in enumerate(step["want"]):
            if want in (se.FITTED, se.CARRIED):
                assert (rec["instance"]["R"][i].reshape(3, 3) == EYE).all() and tuple(rec["instance"]["t"][i]) == fe.T


def rig_tables(script):
    cams = 2 if script.name.startswith("coast") else 1
    n = script.n * cams
    return cams, np.stack([fe.K] * n), np.stack([EYE] * n), np.zeros((n, 3), np.float32), [g * cams for g in range(script.n + 1)]


def rig_present(step, cams):
    """A coast needs a present camera that has not seen the person: of the rig's two, the first is away."""
    return None if step["present"] is None else [0, 1] * len(step["mid"]) if cams == 2 else step["present"]


def rig_state_after(script, k, state):
    """What the named scripts leave in entry 0 after their second step."""
    if k != 1:
        return
    zero = not np.frombuffer(state[0, 0].tobytes(), np.uint8).any()
    if script.name in ("unseen_rejected_is_freed", "coast_above"):
        assert zero, script.name
    if script.name == "seen_rejected_is_kept":
        assert (state[0, 0]["id"], state[0, 0]["tracked"], state[0, 0]["lost"]) == (7, 0, 1)
    if script.name == "coast_on":
        assert (state[0, 0]["id"], state[0, 0]["tracked"], state[0, 0]["lost"]) == (7, 1, 1)


@pytest.mark.parametrize("script", se.scripts(rig=True), ids=lambda s: s.name)
def test_rig_fit_track_ref_gives_the_tracker_literals(script):
    cams, Ks, V, u, rig_begin = rig_tables(script)
    ref = None
    for k, step in enumerate(script.steps):
        tb, frames = frames_of(script, step, cams)
        if ref is None:
            kw = {f: v for f, v in script.prm.items() if f != "min_windows"}
            ref = rf.Tracker(Ks, V, u, rig_begin, *tb.models[0], ANGLE_TABLE, prm=rf.params(**kw))
        n_heads, heads, n_persons, persons = se.rig_inputs(step, PERSON, HEAD)
        if cams == 2:                                   # heads [n_cams, 1]: the rig's second camera has none
            wide = np.zeros((2 * script.n, 1), HEAD)
            wide[::2], persons["best_cam"] = heads, persons["best_cam"] * 2
            heads, n_heads = wide, (np.repeat(n_heads, 2) * np.tile([1, 0], script.n)).astype(np.uint32)
        rec = ref.step(frames, n_heads, heads, n_persons, persons, present=rig_present(step, cams), fit_prm=fr.params(0, 0, (se.GATE, se.GATE)))
        first = rec[:, 0]
        hold_track(script, step, first["status"], first["fit"], first["instance"]["R"], ref.state[:, 0]["tracked"], "rig_fit_track_ref")
        assert (rec[:, 1:]["status"] == se.NONE).all()
        rig_state_after(script, k, ref.state)


# ---------------------------------------------------------------- the trackers' rule, every compare relaxed on its own
def valid_rule(v, relax=None):
    den, num = v.conf[1], v.conf[0]
    l, r = v.mass * den, v.total_mass * num
    lh, ll, rh, rl = l >> 64, l & (2 ** 64 - 1), r >> 64, r & (2 ** 64 - 1)
    total = v.total_mass >= 0 if relax == "total_mass > 0 -> >=" else v.total_mass > 0
    low = ll > rl if relax == "ll >= rl -> >" else ll >= rl
    high = lh >= rh if relax == "lh > rh -> >=" else lh > rh
    if relax == "lh > rh dropped":
        high = False
    equal = True if relax == "lh == rh dropped" else lh == rh
    windows = v.windows > v.min_windows if relax == "windows >= min_windows -> >" else v.windows >= v.min_windows
    return total and (high or (equal and low)) and windows


def angle_rule(rotation, relax=None):
    """The index, or "outside" where the unclamped cast leaves the table (or cannot be made)."""
    lo, hi = {"!(x >= 0.0) -> !(x >= 2.0)": 2.0, "!(x >= 0.0) dropped": None}.get(relax, 0.0), \
        {"x >= 119.0 -> x >= 118.0": 118.0, "x >= 119.0 -> x >= 121.0": 121.0}.get(relax, 119.0)
    x = se.angle_x(rotation)
    if lo is not None and not x >= lo:
        return 0
    if x >= hi:
        return 119
    if not np.isfinite(x) or not 0 <= int(x) < 120:
        return "outside"
    return int(x)


def why_rule(points, e, keep_points, rms_max, relax=None):
    why = 0
    if points <= keep_points if relax == "points < keep_points -> <=" else points < keep_points:
        why |= se.BAD_POINTS
    lim = int(F64(rms_max) * F64(rms_max) * F64(1048576.0)) * points
    if e >= lim if relax == "sum_r2_fixed > lim -> >=" else e > lim:
        why |= se.BAD_RMS
    return why


def jump_rule(fitted, detected, valid, max_jump, relax=None):
    if not valid and relax != "jump test made without a valid or seen detection":
        return 0
    with np.errstate(all="ignore"):
        d = np.float32(fitted).astype(F64) - np.float32(detected).astype(F64)
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        ok = d2 < max_jump * max_jump if relax == "d2 <= jump2 -> <" else d2 <= max_jump * max_jump
    return 0 if ok else se.BAD_JUMP


def track_rows(relax=None):
    """{row: answer} of every tracker row under the local rule with one compare relaxed."""
    out = {v.name: valid_rule(v, relax) for v in se.VALID}
    out.update({name: angle_rule(rotation, relax) for name, rotation, _ in se.ANGLES})
    for s in se.scripts():
        last = s.steps[-1]
        if s.name.startswith(("rms", "keep")):
            out[s.name] = why_rule(last["points"], last["e"], s.prm["keep_points"], s.prm["rms_max"], relax)
        if s.name.startswith("jump"):
            ok = last["support"][0] is None
            out[s.name] = why_rule(last["points"], last["e"], 0, 4096.0, relax) | jump_rule(fe.T, last["mid"][0], ok, s.prm["max_jump"], relax)
        if s.name.startswith("coast"):
            lost = 1
            out[s.name] = not (lost >= s.prm["max_coast"] if relax == "lost > max_coast -> >=" else lost > s.prm["max_coast"])
    for s in se.scripts(rig=True):                      # the rows that only the rig tracker has: every step's answer
        if s.name in ("jump_unseen", "unseen_rejected_is_freed", "seen_rejected_is_kept"):
            out[s.name] = tuple(why_rule(st["points"], st["e"], s.prm["keep_points"], s.prm["rms_max"], relax)
                                | jump_rule(fe.T, st["mid"][0], st["person"], s.prm["max_jump"], relax) for st in s.steps)
    return out


def test_the_local_trackers_rule_gives_the_literals():
    rows = track_rows()
    assert all(rows[v.name] == v.valid for v in se.VALID) and all(rows[name] == index for name, _, index in se.ANGLES)
    for s in se.scripts():
        want = s.steps[-1]["want"][0]
        if s.name.startswith(("rms", "keep", "jump")):
            assert rows[s.name] == (want & 0xF00 if want & 0xFF == se.REJECTED else 0), s.name
        if s.name.startswith("coast"):
            assert rows[s.name] == bool(s.steps[-1]["tracked"][0])
    for s in se.scripts(rig=True):
        if isinstance(rows.get(s.name), tuple):
            assert rows[s.name] == tuple(st["want"][0] & 0xF00 if st["want"][0] & 0xFF == se.REJECTED else 0 for st in s.steps), s.name


@pytest.mark.parametrize("relax", sorted(se.TRACK_FLIPS))
def test_each_relaxed_tracker_compare_flips_exactly_the_rows_that_name_it(relax):
    plain, relaxed = track_rows(), track_rows(relax)
    flipped = {name for name in plain if plain[name] != relaxed[name]}
    assert flipped == se.TRACK_FLIPS[relax] and flipped, (relax, flipped)


# ---------------------------------------------------------------- k_shape_solve's and k_calib_solve's rows
def solve_rows(relax=None):
    """{row: (status, delta bytes)} of the shape and calibration rows: count < min_points, then the local solve."""
    out = {}
    pts, nrm, B = se.shape_model(0)
    inst = se.step_instance(se._SHAPE_CASE)[0]
    for c in se.SHAPES:
        A, b, _, count = sr.instance_sums(se.F65, fe.K, pts, nrm, B[:c.fields], inst, 25.0)
        M = [[F64(A[min(k, l), max(k, l)]) / fr.S for l in range(c.fields)] for k in range(c.fields)]
        if count <= c.min_points if relax == "count < min_points -> <=" else count < c.min_points:
            out[c.name] = (se.SHAPE_FEW_POINTS, None)
            continue
        x = local_solve(M, [F64(v) / fr.S for v in b], c.fields, F64(1.0) + F64(c.lam), relax)
        out[c.name] = (se.SHAPE_SINGULAR, None) if x is None else (se.SHAPE_OK, np.array(x).tobytes())
    for c in se.CALIBS:
        count = 6
        few = count <= c.min_points if relax == "count < min_points -> <=" else count < c.min_points
        out[c.name] = (cr.FEW_POINTS if few else cr.OK, None)
    return out


@pytest.mark.parametrize("n", se.SHAPE_SIZES)
def test_the_restatements_give_the_solve_literals(n):
    pts, nrm, B = se.shape_model(n)
    inst = se.step_instance(se._SHAPE_CASE)
    for c in se.SHAPES:
        rec = sr.shape_step(se.F65[None], fe.K, pts, nrm, B[:c.fields], inst, prm=sr.params(25.0, c.lam, c.min_points))[0]
        assert (rec["status"], rec["points"], rec["sum_r2_fixed"], rec["instances"]) == (c.status, c.points, c.e, 1), c.name
        assert c.delta is None or tuple(rec["delta"][:c.fields]) == c.delta, c.name
        assert solve_rows()[c.name][0] == c.status
    vinst = np.zeros(1, rf.INSTANCE)
    vinst[0] = (0, 0, 1, EYE.reshape(9), fe.T, 1.0, 0)
    for c in se.CALIBS:
        rec = cr.calib_step(se.F65[None, None], fe.K[None], EYE[None], np.zeros((1, 3), np.float32), *se.step_model(se.CALIB_CASE, n or 257), vinst,
                            prm=cr.params(25.0, 0.0, c.min_points, fe.T))[0]
        assert (rec["status"], rec["points"], rec["sum_r2_fixed"], rec["pairs"]) == (c.status, c.points, c.e, 1), c.name
        assert solve_rows()[c.name][0] == c.status


@pytest.mark.parametrize("relax", sorted(se.STEP_FLIPS_SOLVES))
def test_each_relaxed_solve_compare_flips_exactly_the_rows_that_name_it(relax):
    plain, relaxed = solve_rows(), solve_rows(relax)
    flipped = {name for name in plain if plain[name] != relaxed[name]}
    assert flipped == se.STEP_FLIPS_SOLVES[relax] and flipped, (relax, flipped)
