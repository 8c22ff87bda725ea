"""Placed cases for the two decisions that follow the fit family's point correspondence: the STEP RULE of a
fit (count < min_points, every pivot > 0.0, the early exit |x_i| < 1e-6, a coarse refusal that stops the full phase) and the
TRACKERS' RULE (detection validity with its 96-bit compare, the angle index and its clamps, keep_points, the rms limit, the jump
test, max_coast).  Each case puts a value ON a compare, or one representable step to either side of it, and carries its answer as
a literal with the derivation beside it.  No restatement produced the literals; test_fit_step_edges_ref.py holds the restatements
to them and proves each row tight, test_gpu_fit_step_edges.py holds every entry point of the GPU to both.  No GPU code is imported.

THE STEP CASES use the frame of tests/fit_edges.py: 16 x 12, K = [[16, 0, 8], [0, 16, 6], [0, 0, 1]], R = I, scale = 1, and every
point has nm = (0, 0, -1).  Then c = -p.z and the Jacobian of a point at q = p - t is
    J = (0, 0, -1, -q.y, q.x, 0),        res = -p.z * (d / p.z - 1) = -(d - p.z) where p.z is a power of two.
A00 = A11 = A55 = 0, so their pivots are the damping's 1e-9 alone (> 0), and the third pivot is A22 * lam1 + 1e-9 with A22 = count.
At p.z = 64 a point (p.x, p.y) falls on pixel (p.x / 4 + 8, p.y / 4 + 6).

THE TRACKER CASES take the aggregated table of tests/fit_edges.py with only= choosing the kept rows: with schedule (0, 0) and
iterations_tracked = 0 only the last pass runs, so points = P and sum_r2_fixed = E * 2^20 are that table's literals and the pose
comes back as it went in."""
import collections

import numpy as np

import fit_edges as fe

OK, FEW_POINTS, SINGULAR = 0, 1, 2
M20 = 1 << 20
NM = (0.0, 0.0, -1.0)
SIZES = (0, 257, 1025)              # 0: the points alone; staged in LDS with fillers; streamed with fillers

Step = collections.namedtuple("Step", "name pts nrm frame t coarse full gate lam min_points status steps points e still")


def _frame(back, rows=None, pixels=None):
    f = np.full((fe.H, fe.W), back, np.uint16)
    for y, d in (rows or {}).items():
        f[y] = d
    for (x, y), d in (pixels or {}).items():
        f[y, x] = d
    f.setflags(write=False)
    return f


def _step(name, pts, frame, t, sched, gate, lam, min_points, status, steps, points, e, still, nrm=None):
    """still: the pose must come back bit for bit as it went in (no step was taken, or the step was exactly 0); points, e: None
    where the fit moves the pose away from exact arithmetic (held to the restatement alone); nrm: the points' normals where they are
    not NM."""
    nrm = tuple(tuple(float(np.float32(c)) for c in m) for m in (nrm or [NM] * len(pts)))
    return Step(name, tuple(tuple(float(np.float32(c)) for c in p) for p in pts), nrm, frame, tuple(float(c) for c in t), sched[0], sched[1],
                (float(gate[0]), float(gate[1])), float(lam), int(min_points), status, steps, points, e, still)


# ---- the zero pivot.  Six points (+-2048, -+2048, z), z in (0, 64, 128), at t = (0, 0, 8192); every pixel holds 8195.
# They project to (12, 2) and (4, 10) and a fraction of a pixel beside them; the gaps 8195 - (8192 + z) = 3, -61, -125 are inside the
# gate 256.  J3 = -q.y = +-2048 = q.x = J4 for every point and J5 = 0; sum J2 J3 = sum J2 J4 = 0 by symmetry.  A33 = A34 = A44 =
# 6 * 2^22 = 1.5 * 2^24, whose ulp is 2^-28 = 3.7e-9: A33 * 1 + 1e-9 == A33.  f = A34 / A33 = 1 and the fifth pivot is A44 - 1 * A34
# = 0.0 exactly: SINGULAR before any step, the pose as it was.  The last pass keeps all six: at z = 0 res = -3 exactly, e = 9 * 2^20;
# at z = 64 and 128 the quotient 8195 / p.z rounds so that res^2 * 2^20 falls just short of 61^2 * 2^20 and 125^2 * 2^20 and
# truncates to one less (the expression is asserted in test_fit_step_edges_ref.py): e = 2 * (9437184 + 3901751295 + 16383999999).
ZERO_PTS = [(s * 2048.0, -s * 2048.0, z) for z in (0.0, 64.0, 128.0) for s in (1.0, -1.0)]
ZERO_T = (0.0, 0.0, 8192.0)
ZERO_E = 2 * (9437184 + 3901751295 + 16383999999)
F8195 = _frame(8195)
# ---- the zero pivot as the LAST pivot.  After the fifth pivot above is 0.0, f = 0 / 0 makes the sixth NaN, which `piv >= 0.0`
# refuses as `piv > 0.0` does: only a zero in the last place tells the two apart.  Six points (x, +-2048, -+2048), x in (64, 128,
# 192), with nm = (-1, 0, 0) at t = (0, 0, 8192): c = -x < 0, J = (-1, 0, 0, 0, -q.z, q.y), so J4 = J5 = +-2048 and A44 = A45 = A55
# = 6 * 2^22; sum J0 J4 = sum J0 J5 = 0 by symmetry and every other sum but A00 = 6 is 0.  The fifth pivot is A44, f = 1 and the
# sixth is A55 - 1 * A45 = 0.0.  p.z = 6144 (rows 11) and 10240 (row 2); the frame holds p.z itself there, so res = 0, b = 0, e = 0.
# lambda = 2^-52 lifts the pivot above 0: one step with x = 0, after which the early exit leaves.
LAST_PTS = [(x, s * 2048.0, -s * 2048.0) for x in (64.0, 128.0, 192.0) for s in (1.0, -1.0)]
LAST_NRM = [(-1.0, 0.0, 0.0)] * 6
F_LAST = _frame(6144, rows={y: 10240 for y in range(6)})
# ---- the tiny and the negative pivot.  Six points (x_i, a_i * 2^-20, 0) at t = (0, 0, 64) under a frame of 64: res = 0 for all,
# so b = 0 and every solved x is 0 whatever the pivots are.  J3 = -a_i * 2^-20 is a multiple of 2^-20 (nothing truncates), its
# square is below 2^-20 (A33 = 0).  With m = sum a_i: A23 = m * 2^-20, A22 = 6, and the fourth pivot is
#     (0 + 1e-9) - (A23 / (6 + 1e-9)) * A23 = 1e-9 - m^2 * 2^-40 / 6.000000001.
# m = 81 (five points at 13 and one at 16): 1e-9 - 9.9453e-10 = 5.47e-12 > 0, the smallest positive pivot six such points give:
# the step is taken (x = 0: the pose as it was, and the early exit leaves after it).  m = 82 (the last point one step, 2^-20,
# further): 1e-9 - 1.0192e-9 = -1.9e-11 < 0: SINGULAR.
PIVOT_X = (-20.0, -12.0, -4.0, 4.0, 12.0, 20.0)


def _pivot_pts(last):
    return [(x, a * 2.0 ** -20, 0.0) for x, a in zip(PIVOT_X, (13, 13, 13, 13, 13, last))]


F64_ = _frame(64)
# ---- the coarse 3 x 3 solve.  With |n| <= 1 and at most 32768 points a diagonal sum is at most 2^15, whose ulp is 7e-12: the 1e-9
# is never absorbed, so the zero pivot above cannot be formed there.  A NEGATIVE coarse pivot can: the truncation of the
# fixed-point sums breaks A12^2 <= A11 A22.  Six points (x_i, 0, 0) with normals (0, a_i * 2^-20, -1) (squared length 1 + 1.5e-10,
# a unit normal as an f32) under a frame of 64: c = -64, res = 0, J = n.  A11 = 0 (each square is below 2^-20), A12 = -m * 2^-20,
# A22 = 6.  The second pivot is 1e-9, f = A12 / 1e-9, and the third is (6 + 1e-9) - m^2 * 2^-40 / 1e-9: m = 81: 6 - 5.967 = 0.033 > 0,
# one step with x = 0; m = 82: 6 - 6.115 < 0: SINGULAR.
COARSE_PTS = [(x, 0.0, 0.0) for x in PIVOT_X]


def _tilted(last):
    return [(0.0, a * 2.0 ** -20, -1.0) for a in (13, 13, 13, 13, 13, last)]


# a coarse SINGULAR stops the full phase too: the m = 82 normals on six points at (0, 0, 0) (q = 0: J3 = J4 = J5 = 0, so the
# full solve has no sum of theirs to truncate; pixel (8, 6), under 64) and six more with nm = (0, 0, -1) on rows 3 and
# 8 under 264 (gap 200: outside the coarse gate 25, inside the full gate 256).  The coarse solve is the one above: SINGULAR.  The
# full pass would count 12, its third pivot 12 - 6.115 > 0, and would take its steps; it must not run: steps = 0, the pose as it
# was, and the last pass keeps 12 with e = 6 * 200^2 * 2^20.
STOP_PTS = [(0.0, 0.0, 0.0)] * 6 + [(x, y, 0.0) for y in (-10.0, 10.0) for x in (-18.0, 2.0, 18.0)]
F_STOP = _frame(64, rows={3: 264, 8: 264})


# ---- the early exit.  Six points at p.z = 64, symmetric about the axis ((+-18, +-10) and +-(2, 2): the middles of pixels (3 | 12,
# 3 | 8), (8, 6) and (7, 5), so that a step along z moves none of them to another pixel), under a frame of
# 65 (res = -1) or 63 (res = +1): b2 = sum J2 res = +-6, A22 = 6, every other b is 0 (sum q.x = sum q.y = 0) and A23 = A24 = 0, so
# x2 = +-6 / (6 * lam1 + 1e-9) alone is not 0, in the coarse 3 x 3 and in the full 6 x 6 solve alike.  lam1 = 1 + lambda.
# lambda = 999999.0: lam1 = 1e6, 6e6 + 1e-9 rounds up one ulp (9.3e-10), x2 is one step below 1e-6: small, the phase leaves
# after 1 step.  lambda = nextafter(999999.0, 0): 6 * lam1 + 1e-9 rounds to 6e6 and x2 == 1e-6 exactly, which is NOT small: a second
# step follows, whose x2 = 1e-6 * (1 - 1e-6) is small: 2 steps.  After k steps p.z = 64 +- k * 1e-6, res = -+(1 - k * 1e-6) and
# e = 6 * trunc((1 - k * 1e-6)^2 * 2^20) = 6 * 1048573 (k = 1) or 6 * 1048571 (k = 2).
EXIT_PTS = [(18.0, 10.0, 0.0), (-18.0, -10.0, 0.0), (18.0, -10.0, 0.0), (-18.0, 10.0, 0.0), (2.0, 2.0, 0.0), (-2.0, -2.0, 0.0)]
LAM_BELOW = 999999.0
LAM_ON = float(np.nextafter(999999.0, 0.0))
# ---- a coarse early exit does not stop the full phase.  Twelve points: the six above under 65 and six more on rows 4 and 7 under
# 264 (gap 200: outside the coarse gate 25, inside the full gate 256).  Coarse, lambda = 999999: x2 one step below 1e-6, the coarse
# phase leaves after 1 of its 3 steps.  Full: b2 = 6 + 6 * 200 = 1206, A22 = 12, x2 = 1206 / 12e6 = 1e-4 is not small and stays so: both
# full steps run.  steps = 1 + 2.  The model is symmetric, x3 = x4 = x5 = 0 exactly and R stays the identity.
THEN_PTS = EXIT_PTS + [(10.0, 6.0, 0.0), (-10.0, -6.0, 0.0), (10.0, -6.0, 0.0), (-10.0, 6.0, 0.0), (6.0, -6.0, 0.0), (-6.0, 6.0, 0.0)]
F_THEN = _frame(65, rows={4: 264, 7: 264})
# ---- FEW_POINTS.  The six points under 65, but pixel (3, 3) holds 94 (gap 30: outside gate 25, inside 256).
#   coarse refusal: gate (25, 256).  The coarse pass counts 5 < 6: FEW_POINTS, and the full phase, whose gate would count 6, must
#   not run: steps = 0, the pose as it was; the last pass (gate 256) keeps 6: e = (5 * 1 + 30^2) * 2^20.
#   full refusal: gate (256, 25), schedule (0, 2): the full pass counts 5: FEW_POINTS, steps 0; the last pass keeps 5: e = 5 * 2^20.
F_FEW = _frame(65, pixels={(3, 3): 94})
F65, F63 = _frame(65), _frame(63)
# ---- min_points on the count.  The six points under 65, lambda = 0: count = 6.  min_points = 6: the step is taken, x2 = 6 / (6 +
# 1e-9) = 1 - 1.7e-10, t.z = 65 - 1.7e-10 (65.0 as an f32); the last pass: res = 1.7e-10, e = 0.  min_points = 7: FEW_POINTS, no
# step, e = 6 * 2^20.

STEPS = (
    _step("zero_pivot", ZERO_PTS, F8195, ZERO_T, (0, 2), (256, 256), 0.0, 6, SINGULAR, 0, 6, ZERO_E, True),
    # lambda = 2^-52: A33 * lam1 rounds up, the fifth pivot is a few ulps of 2^24 above 0: both steps are taken (the step is huge,
    # so points and e are the restatement's).
    _step("zero_pivot_damped", ZERO_PTS, F8195, ZERO_T, (0, 2), (256, 256), 2.0 ** -52, 6, OK, 2, None, None, False),
    _step("last_pivot_zero", LAST_PTS, F_LAST, ZERO_T, (0, 2), (256, 256), 0.0, 6, SINGULAR, 0, 6, 0, True, nrm=LAST_NRM),
    _step("last_pivot_zero_damped", LAST_PTS, F_LAST, ZERO_T, (0, 2), (256, 256), 2.0 ** -52, 6, OK, 1, 6, 0, True, nrm=LAST_NRM),
    _step("tiny_pivot", _pivot_pts(16), F64_, fe.T, (0, 2), (25, 25), 0.0, 6, OK, 1, 6, 0, True),
    _step("negative_pivot", _pivot_pts(17), F64_, fe.T, (0, 2), (25, 25), 0.0, 6, SINGULAR, 0, 6, 0, True),
    _step("coarse_positive_pivot", COARSE_PTS, F64_, fe.T, (2, 0), (25, 25), 0.0, 6, OK, 1, 6, 0, True, nrm=_tilted(16)),
    _step("coarse_negative_pivot", COARSE_PTS, F64_, fe.T, (2, 0), (25, 25), 0.0, 6, SINGULAR, 0, 6, 0, True, nrm=_tilted(17)),
    _step("coarse_singular_stops", STOP_PTS, F_STOP, fe.T, (2, 2), (25, 256), 0.0, 6, SINGULAR, 0, 12, 240000 * M20, True, nrm=_tilted(17) + [NM] * 6),
    _step("coarse_exit_below", EXIT_PTS, F65, fe.T, (3, 0), (25, 25), LAM_BELOW, 6, OK, 1, 6, 6 * 1048573, False),
    _step("coarse_exit_on", EXIT_PTS, F65, fe.T, (3, 0), (25, 25), LAM_ON, 6, OK, 2, 6, 6 * 1048571, False),
    _step("coarse_exit_below_negative", EXIT_PTS, F63, fe.T, (3, 0), (25, 25), LAM_BELOW, 6, OK, 1, 6, 6 * 1048573, False),
    _step("coarse_exit_on_negative", EXIT_PTS, F63, fe.T, (3, 0), (25, 25), LAM_ON, 6, OK, 2, 6, 6 * 1048571, False),
    _step("full_exit_below", EXIT_PTS, F65, fe.T, (0, 3), (25, 25), LAM_BELOW, 6, OK, 1, 6, 6 * 1048573, False),
    _step("full_exit_on", EXIT_PTS, F65, fe.T, (0, 3), (25, 25), LAM_ON, 6, OK, 2, 6, 6 * 1048571, False),
    _step("full_exit_below_negative", EXIT_PTS, F63, fe.T, (0, 3), (25, 25), LAM_BELOW, 6, OK, 1, 6, 6 * 1048573, False),
    _step("full_exit_on_negative", EXIT_PTS, F63, fe.T, (0, 3), (25, 25), LAM_ON, 6, OK, 2, 6, 6 * 1048571, False),
    _step("coarse_exit_then_full", THEN_PTS, F_THEN, fe.T, (3, 2), (25, 256), LAM_BELOW, 6, OK, 3, 12, None, False),
    _step("coarse_few_stops", EXIT_PTS, F_FEW, fe.T, (1, 2), (25, 256), 0.0, 6, FEW_POINTS, 0, 6, 905 * M20, True),
    _step("full_few", EXIT_PTS, F_FEW, fe.T, (0, 2), (256, 25), 0.0, 6, FEW_POINTS, 0, 5, 5 * M20, True),
    _step("coarse_min_points_on", EXIT_PTS, F65, fe.T, (1, 0), (25, 25), 0.0, 6, OK, 1, 6, 0, False),
    _step("coarse_min_points_above", EXIT_PTS, F65, fe.T, (1, 0), (25, 25), 0.0, 7, FEW_POINTS, 0, 6, 6 * M20, True),
    _step("full_min_points_on", EXIT_PTS, F65, fe.T, (0, 1), (25, 25), 0.0, 6, OK, 1, 6, 0, False),
    _step("full_min_points_above", EXIT_PTS, F65, fe.T, (0, 1), (25, 25), 0.0, 7, FEW_POINTS, 0, 6, 6 * M20, True),
)
STEP_BY_NAME = {s.name: s for s in STEPS}
assert len(STEP_BY_NAME) == len(STEPS)
FULL_ONLY = tuple(s.name for s in STEPS if s.coarse == 0)      # what a carried start (schedule (0, iterations_tracked)) can run


def step_model(case, n):
    """(points [n, 3] f32, normals [n, 3] f32): the case's points at the indices of fit_edges.slots(n) -- the first and last lane of
    a wave, the last lane of the workgroup, the second stride, either side of the LDS staging budget -- among fit_edges.FILLER
    points, which face away and take no part at any pose."""
    n = n or len(case.pts)
    assert n >= len(case.pts)
    items = [fe.FILLER] * n
    for i, p, m in zip(fe.slots(n), case.pts, case.nrm):
        items[i] = (p, m)
    return fe.model_of(items)


def step_instance(case, frame=0, model=0):
    return np.array([fe.instance(frame, model, case.t, flags=0x5E0000)], fe.INST_DTYPE)


def step_tracker_inputs(case):
    """fit_edges.tracker_inputs with mid_point = the case's t: the exact start R = I, t of a detected step."""
    poses, support, kw = fe.tracker_inputs()
    poses["mid_point"] = case.t
    return poses, support, kw


# ================================================================ the trackers' rule
GATE = 25.0
N_TRACK = 257
# ---- the rms limit: sum_r2_fixed > (int64)(rms_max^2 * 2^20) * points.  A selection whose E / P is a perfect square r^2: at
# rms_max = r the limit is r^2 * 2^20 * P = E * 2^20 exactly, which is not above itself: accepted.  At nextafter(r, 0) the product
# rms_max^2 * 2^20 lies just below r^2 * 2^20 and the cast truncates it to r^2 * 2^20 - 1: E * 2^20 > limit: BAD_RMS.
#   pz_on alone: P = 1, E = 4, r = 2.    x_below_w (64) + pixel_one (0) + c_tiny (0) + graze_on (0): P = 4, E = 64, r = 4.
Rms = collections.namedtuple("Rms", "only points e rms_max")
RMS = (Rms(("pz_on",), 1, 4 * M20, 2.0), Rms(("x_below_w", "pixel_one", "c_tiny", "graze_on"), 4, 64 * M20, 4.0))
# ---- the jump test on a carried step: the fit of step 1 stands at T = (0, 0, 64) and step 2 returns it unchanged; the detection of
# step 2 at (3, 4, 64) lies at d2 = 9 + 16 + 0 = 25 = max_jump^2 with max_jump = 5: accepted.  64 + 2^-17 is the next f32 above 64:
# d2 = 25 + 2^-34 > 25: BAD_JUMP.  With a support that is not valid the test is not made: CARRIED.  NaN fails `d2 <= jump2`.
MAX_JUMP = 5.0
JUMP_ON, JUMP_BEYOND = (3.0, 4.0, 64.0), (3.0, 4.0, 64.0 + 2.0 ** -17)
JUMP_NAN = (float("nan"), 4.0, 64.0)
# ---- detection validity: total_mass > 0, mass * conf_den >= total_mass * conf_num in 96 bits, windows >= min_windows.
# Each row: (name, conf, min_windows, mass, total_mass, windows, valid); the products are written out as Python ints.  Only the
# windows rows run at a min_windows above 0, so that no other row sits on that compare.
Valid = collections.namedtuple("Valid", "name conf min_windows mass total_mass windows valid")
M50 = (2 ** 64 - 1) // 50            # 368934881474191032; 50 * M50 = 18446744073709551600 = 2^64 - 16
assert M50 == 368934881474191032 and 50 * M50 == 18446744073709551600
VALID = (
    Valid("total_zero", (0, 1), 0, 0, 0, 1, False),                     # 0 * 1 >= 0 * 0 holds; total_mass > 0 alone refuses
    Valid("conf_zero_mass_zero", (0, 1), 0, 0, 1, 1, True),             # 0 * 1 = 0 >= 1 * 0 = 0
    Valid("windows_on", (1, 50), 3, 1, 1, 3, True),
    Valid("windows_below", (1, 50), 3, 1, 1, 2, False),
    # conf = 1 / 50, the default.  50 * M50 = 2^64 - 16 = total * 1: both high words 0, low words equal: valid
    Valid("low_equal_50", (1, 50), 0, M50, 18446744073709551600, 1, True),
    Valid("low_below_50", (1, 50), 0, M50, 18446744073709551601, 1, False),
    # conf = 3 / 4: the products leave the low word.
    # mass * 4 = 3 * 2^61 * 4 = 27670116110564327424 = 2^64 + 2^63 = total * 3 = 2^63 * 3: high 1 == 1, low 2^63 == 2^63: valid
    Valid("high_equal_low_equal", (3, 4), 0, 3 * 2 ** 61, 2 ** 63, 1, True),
    # mass * 4 = (2^62 + 1) * 4 = 2^64 + 4; total * 3 = 6148914691236517206 * 3 = 2^64 + 2: high 1 == 1, low 4 >= 2: valid
    Valid("high_equal_low_above", (3, 4), 0, 2 ** 62 + 1, 6148914691236517206, 1, True),
    # total * 3 = 6148914691236517207 * 3 = 2^64 + 5: high 1 == 1, low 4 < 5: not valid
    Valid("high_equal_low_below", (3, 4), 0, 2 ** 62 + 1, 6148914691236517207, 1, False),
    # mass * 4 = 2^63 * 4 = 2^65: high 2, low 0; total * 3 = 2^63 * 3 = 2^64 + 2^63: high 1, low 2^63.  lh > rh, ll < rl: valid
    Valid("high_above_low_below", (3, 4), 0, 2 ** 63, 2 ** 63, 1, True),
    # mass * 4 = 3 * 2^61 * 4 = 2^64 + 2^63: high 1, low 2^63; total * 3 = 12297829382473034411 * 3 = 2^65 + 1: high 2, low 1.
    # lh < rh, ll > rl: not valid
    Valid("high_below_low_above", (3, 4), 0, 3 * 2 ** 61, 12297829382473034411, 1, False),
)
assert 6148914691236517206 * 3 == 2 ** 64 + 2 and 6148914691236517207 * 3 == 2 ** 64 + 5 and 12297829382473034411 * 3 == 2 ** 65 + 1
assert all((v.mass * v.conf[1] >= v.total_mass * v.conf[0] and v.total_mass > 0 and v.windows >= v.min_windows) == v.valid for v in VALID)
assert all(0 <= v.mass < 2 ** 64 and 0 <= v.total_mass < 2 ** 64 for v in VALID)
VALID_CONFS = tuple(sorted({(v.conf, v.min_windows) for v in VALID}))
# ---- the angle index: x = rotation / 3.14159 * 60 + 60.5; !(x >= 0) -> 0, x >= 119 -> 119, else (int)x.  (name, rotation, index).
# rotation = -3.14159: x = 0.5 -> 0.  3.14159: x = 120.5 -> 119 (the clamp).  nextafter(3.14159, 0): x just below 120.5 -> 119 (the
# clamp again).  -4.0: x = -15.9 -> 0 (the lower clamp; (int)x would be -15).  +inf -> 119, -inf -> 0, NaN -> 0 (`!(x >= 0)`).
# k * BIN with BIN = 3.14159 / 60: x = k + 60.5 up to rounding, -> k + 60 for k in -60 .. 58; k = 59: x = 119.5 -> the clamp's 119,
# as (int)x would give; k = 60: x = 120.5 -> 119 where (int)x is 120, one past the table.
BIN = 3.14159 / 60.0
ANGLES = (("minus_pi", -3.14159, 0), ("below_pi", float(np.nextafter(3.14159, 0.0)), 119), ("pi", 3.14159, 119), ("minus_four", -4.0, 0),
          ("plus_inf", float("inf"), 119), ("minus_inf", float("-inf"), 0), ("nan", float("nan"), 0)) + \
    tuple((f"grid_{k}", k * BIN, min(k + 60, 119)) for k in (-60, -59, -1, 0, 1, 58, 59, 60))
# No row sits ON x == 0.0 or x == 119.0: (int)x is 0 on [0, 1) and 119 on [119, 120), the very values the clamps give, so where
# exactly in (-1, 1] the lower and in (118, 120] the upper compare stands cannot be observed; what can be is that they stand no
# further out (minus_four, pi, grid_60: an index outside the table) and no further in (grid_-59, grid_58).


def angle_x(rotation):
    with np.errstate(all="ignore"):
        return np.float64(rotation) / np.float64(3.14159) * np.float64(60.0) + np.float64(60.5)


def tracker_table(only):
    """The aggregated table of fit_edges at gate 25 with the kept rows `only`: points = P, e = E * 2^20."""
    return fe.aggregated(N_TRACK, GATE, only=tuple(only))


def support_of(rows):
    """dh_support records of Valid rows (or one valid record per None)."""
    _, one, _ = fe.tracker_inputs()
    out = np.zeros(len(rows), one.dtype)
    for i, v in enumerate(rows):
        out[i] = one[0]
        if v is not None:
            out[i]["mass"], out[i]["total_mass"], out[i]["windows"] = v.mass, v.total_mass, v.windows
    return out


# ================================================================ the trackers' scripts: what both test files run, step after step
NONE, FITTED, CARRIED, REJECTED, ABSENT = 0, 1, 2, 3, 4
BAD_STATUS, BAD_POINTS, BAD_RMS, BAD_JUMP = 0x100, 0x200, 0x400, 0x800
HUGE = 0xFFFFFFFF
BELIEVE = dict(iterations_tracked=0, keep_points=0, rms_max=4096.0, max_jump=4096.0, min_windows=0)
# (min_windows = 0 with windows = 1, mass = total_mass = 1 at conf 1 / 50: the support of fit_edges.tracker_inputs is valid and sits
# on none of the validity compares, so a row that is not about validity cannot flip under them.)
KEEP_ONLY = RMS[1].only                       # P = 4, E = 64
Script = collections.namedtuple("Script", "name only prm n steps")
# a step: dict(mid [n][3], rotation [n][3] or None, support rows [n] (Valid or None), present (None or [n]), empty (an all-zero
# frame), person (the rig form: False = no person record), want [n] statuses, points, e (the literals of an instance that was
# fitted), tracked [n] (the state after the step) or None)


def _st(n, mid=None, rotation=None, support=None, present=None, empty=False, person=True, want=(), points=None, e=None, tracked=None):
    return dict(mid=[fe.T] * n if mid is None else mid, rotation=rotation, support=support or [None] * n, present=present, empty=empty,
                person=person, want=list(want), points=points, e=e, tracked=tracked)


NOT_VALID = Valid("not_valid", (1, 50), 0, 0, 0, 1, False)     # total_mass = 0


def scripts(rig=False):
    """The scripts of the FitTracker (rig=False: one camera per row) or of the RigFitTracker (rig=True: one rig of one identity camera
    per row; the rows that turn on detection validity do not exist there: a person record is a detection)."""
    out = []
    for k, r in enumerate(RMS):
        for what, rms, want in (("on", r.rms_max, FITTED), ("below", float(np.nextafter(r.rms_max, 0.0)), REJECTED | BAD_RMS)):
            out.append(Script(f"rms_{k}_{what}", r.only, dict(BELIEVE, rms_max=rms), 1, [_st(1, want=[want], points=r.points, e=r.e)]))
    P, E = RMS[1].points, RMS[1].e
    for what, keep, want in (("on", P, FITTED), ("above", P + 1, REJECTED | BAD_POINTS)):
        out.append(Script(f"keep_{what}", KEEP_ONLY, dict(BELIEVE, keep_points=keep), 1, [_st(1, want=[want], points=P, e=E)]))
    jump = dict(BELIEVE, max_jump=MAX_JUMP)
    first = _st(1, want=[FITTED], points=P, e=E, tracked=[1])
    for what, mid, want in (("on", JUMP_ON, CARRIED), ("beyond", JUMP_BEYOND, REJECTED | BAD_JUMP), ("nan", JUMP_NAN, REJECTED | BAD_JUMP)):
        out.append(Script(f"jump_{what}", KEEP_ONLY, jump, 1, [first, _st(1, mid=[mid], want=[want], points=P, e=E)]))
    if rig:         # an unseen entry: no jump test; rejected (an empty frame under keep_points = P), it is freed
        out.append(Script("jump_unseen", KEEP_ONLY, jump, 1, [first, _st(1, mid=[JUMP_BEYOND], person=False, want=[CARRIED], points=P, e=E, tracked=[1])]))
        keep = dict(jump, keep_points=P)
        out.append(Script("unseen_rejected_is_freed", KEEP_ONLY, keep, 1,
                          [first, _st(1, person=False, empty=True, want=[REJECTED | BAD_POINTS], points=0, e=0, tracked=[0])]))
        out.append(Script("seen_rejected_is_kept", KEEP_ONLY, keep, 1,
                          [first, _st(1, empty=True, want=[REJECTED | BAD_POINTS], points=0, e=0, tracked=[0])]))
    else:           # a detection that is not valid: the jump test is not made
        out.append(Script("jump_invalid", KEEP_ONLY, jump, 1,
                          [first, _st(1, mid=[JUMP_BEYOND], support=[NOT_VALID], want=[CARRIED], points=P, e=E, tracked=[1])]))
        for conf, min_windows in VALID_CONFS:
            rows = [v for v in VALID if (v.conf, v.min_windows) == (conf, min_windows)]
            out.append(Script(f"valid_{conf[0]}_{conf[1]}_{min_windows}", KEEP_ONLY, dict(BELIEVE, conf=conf, min_windows=min_windows), len(rows),
                              [_st(len(rows), support=rows, want=[FITTED if v.valid else NONE for v in rows], points=P, e=E)]))
    n = len(ANGLES)
    out.append(Script("angles", KEEP_ONLY, dict(BELIEVE, keep_points=HUGE), n,
                      [_st(n, rotation=[(a[1],) * 3 for a in ANGLES], want=[REJECTED | BAD_POINTS] * n)]))    # (a turned start: the fit's sums are not the table's)
    for what, coast, kept in (("on", 1, 1), ("above", 0, 0)):        # one step away: lost = 1 == max_coast is kept, 1 > 0 is dropped
        out.append(Script(f"coast_{what}", KEEP_ONLY, dict(BELIEVE, max_coast=coast), 1,
                          [first, _st(1, present=[0], person=False, want=[ABSENT], tracked=[kept])]))
    return out


def poses_of(step, dtype):
    out = np.zeros(len(step["mid"]), dtype)
    out["mid_point"] = step["mid"]
    if step["rotation"] is not None:
        out["rotation"] = step["rotation"]
    return out


def rig_inputs(step, person_dtype, head_dtype, persons_per_rig=16):
    """(n_heads [n], heads [n, 1], n_persons [n], persons [n, 16]) of n rigs of one camera each: rig g's person 0 (id 7, seen by its
    one camera, world = the step's mid, head 0 of camera g with the step's rotation), or no person."""
    n = len(step["mid"])
    n_heads, heads = np.zeros(n, np.uint32), np.zeros((n, 1), head_dtype)
    n_persons, persons = np.zeros(n, np.uint32), np.zeros((n, persons_per_rig), person_dtype)
    if step["person"]:
        n_heads[:], n_persons[:] = 1, 1
        heads[:, 0]["pose"] = poses_of(step, heads.dtype["pose"])
        p = persons[:, 0]
        p["views"], p["mass"], p["n_views"], p["world"], p["id"], p["best_cam"] = 1, 100, 1, step["mid"], 7, np.arange(n)
    return n_heads, heads, n_persons, persons


# ================================================================ which rows sit ON which compare
# relaxation of one compare -> the rows whose answer changes under it, and no others.  test_fit_step_edges_ref.py proves the whole
# table on local copies of both rules; DESIGN.md section 18e lists it.  Every step case whose first pass keeps 6 points runs at
# min_points = 6 (the host refuses less), so all of those sit on `count < min_points` as well as on their own compare.
_ON_COUNT = {s.name for s in STEPS if s.status != FEW_POINTS}
STEP_FLIPS = {
    "piv > 0.0 -> >=": {"last_pivot_zero"},
    "abs(x) < 1e-6 -> <=": {"coarse_exit_on", "coarse_exit_on_negative", "full_exit_on", "full_exit_on_negative"},
    "count < min_points -> <=": _ON_COUNT,
    "coarse FEW_POINTS stop dropped": {"coarse_few_stops"},
    "coarse SINGULAR stop dropped": {"coarse_singular_stops"},
}
TRACK_FLIPS = {
    # (the rig tracker's two rows that reject an empty frame under keep_points = P sit on both of these as well: 0 > lim * 0 in
    # their second step, P < P in their first)
    "sum_r2_fixed > lim -> >=": {"rms_0_on", "rms_1_on", "unseen_rejected_is_freed", "seen_rejected_is_kept"},
    "points < keep_points -> <=": {"keep_on", "unseen_rejected_is_freed", "seen_rejected_is_kept"},
    "d2 <= jump2 -> <": {"jump_on"},
    "jump test made without a valid or seen detection": {"jump_invalid", "jump_unseen"},
    "total_mass > 0 -> >=": {"total_zero"},
    "ll >= rl -> >": {"conf_zero_mass_zero", "low_equal_50", "high_equal_low_equal"},
    "lh > rh -> >=": {"low_below_50", "high_equal_low_below"},
    "lh > rh dropped": {"high_above_low_below"},
    "lh == rh dropped": {"high_below_low_above"},
    "windows >= min_windows -> >": {"windows_on"},
    "x >= 119.0 -> x >= 118.0": {"grid_58"},
    "x >= 119.0 -> x >= 121.0": {"pi", "below_pi", "grid_60"},
    "!(x >= 0.0) -> !(x >= 2.0)": {"grid_-59"},
    "!(x >= 0.0) dropped": {"minus_four", "minus_inf", "nan"},
    "lost > max_coast -> >=": {"coast_on"},
}


# ================================================================ the shape step's and the calibration step's solves
# k_shape_solve and k_calib_solve make the same two decisions on a subject's or a camera's sums: count < min_points, then
# fit_solve_tri.  SHAPE_PTS: 256 points at p.z = 64, one in the middle of every pixel of the frame and 64 of them twice, under a
# frame of 65 (res = -1, e = 256 * 2^20).  A field (0, 0, 256) -- DH_SHAPE_MAX_FIELD -- gives J = nm . B = -256 for every point.
#   Two equal fields: A00 = A01 = A11 = 256 * 2^16 = 2^24, whose ulp is 2^-28: A00 * 1 + 1e-9 == A00, f = 1 and the second and LAST
#   pivot is A11 - 1 * A01 = 0.0: SINGULAR, delta 0.  lambda = 2^-52 lifts it: OK.
#   One field, min_points = 256 = count: OK with delta = b0 / A00 = 2^16 / 2^24 = 2^-8 (b0 = sum J res = 256 * 256); 257: FEW_POINTS.
# The calibration step cannot take the zero pivot here: its rotation columns are (q x n) / DH_CALIB_ARM_UNIT with q the point's arm
# from the pivot, at most 2048 * sqrt(3) + 4096 = 7643 mm (DH_CALIB_MAX_ARM per component, DH_FIT_MAX_EXTENT), so |J| < 120 and a
# diagonal sum reaches 2^24 only from about 1170 points on, beyond the 1025 points of a test; its min_points rows run on the six
# EXIT_PTS under 65 with the pivot at T.
SHAPE_PTS = [(4.0 * (i % 16) - 30.0, 4.0 * ((i // 16) % 12) - 22.0, 0.0) for i in range(256)]
SHAPE_OK, SHAPE_FEW_POINTS, SHAPE_SINGULAR = 0, 1, 2
Shape = collections.namedtuple("Shape", "name fields lam min_points status points e delta")
SHAPES = (
    Shape("shape_zero_pivot", 2, 0.0, 256, SHAPE_SINGULAR, 256, 256 * M20, (0.0, 0.0)),
    Shape("shape_zero_pivot_damped", 2, 2.0 ** -52, 256, SHAPE_OK, 256, 256 * M20, None),
    Shape("shape_min_points_on", 1, 0.0, 256, SHAPE_OK, 256, 256 * M20, (2.0 ** -8,)),
    Shape("shape_min_points_above", 1, 0.0, 257, SHAPE_FEW_POINTS, 256, 256 * M20, (0.0,)),
)
SHAPE_SIZES = (0, 1025)
_SHAPE_CASE = _step("shape", SHAPE_PTS, F65, fe.T, (0, 0), (25, 25), 0.0, 6, OK, 0, 256, 256 * M20, True)
CALIB_CASE = STEP_BY_NAME["full_min_points_on"]
Calib = collections.namedtuple("Calib", "name min_points status points e")
CALIBS = (Calib("calib_min_points_on", 6, 0, 6, 6 * M20), Calib("calib_min_points_above", 7, 1, 6, 6 * M20))
STEP_FLIPS_SOLVES = {"piv > 0.0 -> >=": {"shape_zero_pivot"},
                     "count < min_points -> <=": {"shape_zero_pivot", "shape_zero_pivot_damped", "shape_min_points_on", "calib_min_points_on"}}


def shape_model(n):
    """(points, normals, fields [2, n, 3]): SHAPE_PTS among fillers, and two equal fields (0, 0, 256) (a one-field case takes the first)."""
    pts, nrm = step_model(_SHAPE_CASE, n)
    B = np.zeros((2, len(pts), 3), np.float32)
    B[..., 2] = 256.0
    return pts, nrm, B
