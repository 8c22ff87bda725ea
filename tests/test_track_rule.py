"""The live-tracking rule of dh_tracker_step (depthhead_amd/csrc/dh_track.h, the header k_track is built from) against a
Python restatement of the reference's live loop, examples/live_prediction.rs:79-101, at its boundaries: an L1 distance of
exactly 100.0f and its f32 neighbours, a stored z of exactly 500.0f, the first frame, -0.0, a large jump while the stored z
is below 500, and all four flag combinations.  The header is compiled by plain g++ (tests/host/track_check.cpp), under
ASan / UBSan."""
import numpy as np

import host_program as hp

PREV, SLUG = 1, 2
f32 = np.float32


def ref_update(flags, mid, stored, has_rot):
    """live_prediction.rs:79-101 for one camera: (stored midpoint after the step, next mask, has_rot after, mask before)."""
    mid = [f32(v) for v in mid]
    stored = [f32(v) for v in stored]
    prev, sluggish = bool(flags & PREV), bool(flags & SLUG)
    # :79-86 (guess offered to this step) and :101 (rotation guess after the first frame)
    before = (1 if prev and stored[2] > f32(500.0) else 0) | (2 if prev and has_rot else 0)
    # :92-99, f32 arithmetic summed left to right
    d = (abs(f32(mid[0] - stored[0])) + abs(f32(mid[1] - stored[1]))) + abs(f32(mid[2] - stored[2]))
    if not sluggish or f32(d) < f32(100.0) or stored[2] < f32(500.0):
        stored = mid
    after = (1 if prev and stored[2] > f32(500.0) else 0) | (2 if prev else 0)
    return stored, after, 1, before


def bits(v):
    return int(np.array(v, dtype=np.float32).view(np.uint32))


def cases():
    below, above = np.nextafter(f32(100), f32(0)), np.nextafter(f32(100), f32(1000))
    z5lo, z5hi = np.nextafter(f32(500), f32(0)), np.nextafter(f32(500), f32(1000))
    base = [
        # (new midpoint, stored midpoint, has_rot)
        ((100.0, 0.0, 600.0), (0.0, 0.0, 600.0), 1),          # L1 exactly 100: held
        ((below, 0.0, 600.0), (0.0, 0.0, 600.0), 1),          # just below: moves
        ((above, 0.0, 600.0), (0.0, 0.0, 600.0), 1),          # just above: held
        ((0.0, 0.0, 700.0), (0.0, 0.0, 600.0), 1),            # z difference exactly 100
        ((30.0, 30.0, 640.0), (0.0, 0.0, 600.0), 1),          # 30 + 30 + 40 = 100
        ((-30.0, 30.1, 639.9), (0.0, 0.0, 600.0), 1),         # sums that round near 100
        ((33.333336, 33.333332, 633.33333), (0.0, 0.0, 600.0), 1),
        ((0.1, 0.2, 599.7), (0.0, 0.0, 500.0), 1),            # stored z exactly 500: not < 500, guess not offered
        ((400.0, 0.0, 900.0), (0.0, 0.0, 500.0), 1),          # far jump at stored z = 500: held
        ((400.0, 0.0, 900.0), (0.0, 0.0, z5lo), 1),           # stored z just below 500: moves
        ((400.0, 0.0, 900.0), (0.0, 0.0, z5hi), 1),           # stored z just above 500: held, guess offered
        ((12.0, -40.0, 800.0), (0.0, 0.0, 0.0), 0),           # first frame
        ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0),                # first frame, empty result
        ((-0.0, -0.0, 600.0), (0.0, 0.0, 600.0), 1),          # -0.0 is stored as -0.0
        ((0.0, 0.0, 600.0), (-0.0, -0.0, 600.0), 1),
        ((-0.0, 0.0, -0.0), (0.0, -0.0, 0.0), 0),
        ((1000.0, -1000.0, 2500.0), (0.0, 0.0, 400.0), 1),    # large jump while stored z < 500: moves
        ((1000.0, -1000.0, 2500.0), (5.0, 5.0, 800.0), 1),    # large jump from z 800: held
        ((0.0, 0.0, 400.0), (0.0, 0.0, 800.0), 1),            # dropping below 500 by a far step: held
        ((0.0, 0.0, 750.0), (0.0, 0.0, 800.0), 1),            # ... by a near one: moves
    ]
    rs = np.random.RandomState(7)
    for _ in range(200):
        s = rs.uniform(-300, 300, 3).astype(np.float32)
        s[2] = rs.choice([rs.uniform(0, 1200), 500.0, 0.0])
        m = s + rs.uniform(-60, 60, 3).astype(np.float32)
        base.append((tuple(m), tuple(s), int(rs.randint(0, 2))))
    return [(fl,) + c for fl in (0, PREV, SLUG, PREV | SLUG) for c in base]


def _build_and_run(tmp_path, sanitize):
    exe = hp.build(tmp_path, "track_check", [hp.host("track_check.cpp")], sanitize, ("-I" + hp.CSRC,))
    cs = cases()
    lines = "".join("%x %x %x %x %x %x %x %x\n" % ((fl,) + tuple(bits(v) for v in m) + tuple(bits(v) for v in s) + (hr,))
                    for fl, m, s, hr in cs)
    run = hp.run(exe, stdin=lines, timeout=120)
    out = run.stdout.strip().splitlines()
    assert len(out) == len(cs)
    for (fl, m, s, hr), line in zip(cs, out):
        f = line.split()
        got_st = [int(x, 16) for x in f[:3]]
        ref_st, ref_mask, ref_hr, ref_before = ref_update(fl, m, s, hr)
        assert got_st == [bits(v) for v in ref_st], (fl, m, s, hr, line)
        assert (int(f[3]), int(f[4]), int(f[5])) == (ref_mask, ref_hr, ref_before), (fl, m, s, hr, line)


def test_track_rule_matches_the_live_loop(tmp_path):
    _build_and_run(tmp_path, None)


def test_track_rule_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "address,undefined")


def test_boundary_cases_decide_both_ways():
    """The restatement itself: the boundary cases exercise both outcomes of every comparison."""
    held = moved = 0
    for fl, m, s, hr in [c for c in cases() if c[0] == SLUG][:20]:
        st, _, _, _ = ref_update(fl, m, s, hr)
        if [bits(v) for v in st] == [bits(v) for v in s] and [bits(v) for v in m] != [bits(v) for v in s]:
            held += 1
        else:
            moved += 1
    assert held >= 5 and moved >= 5, (held, moved)
