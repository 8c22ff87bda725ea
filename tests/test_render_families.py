"""The renderer's restatement (tests/render_ref.py) on the edge families of tests/render_families.py, held to a second statement
of the rule of DESIGN.md section 17 that shares nothing with it but the f32 vertex stage: coverage by a nudged sample point in
Python integers, depth by exact rational interpolation.  Where the two disagree the rule in include/depthhead_hip.h decides who
is wrong.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import render_families as rf
import render_ref as rr

# Coverage, phrased without edge ownership: the centre P is covered when P + (eps, eps^2) lies strictly inside all three edges
# for every small enough eps > 0.  With eps = 1 / S the edge function of a -> b there, times S^2, is
#     S^2 E(P) - S dy + dx            (E, dx, dy integers; dx, dy the edge's direction in a triangle of positive area).
# |dx|, |dy| <= 2^21 (snapped coordinates within +-2^20), so with S = 2^23 > 2^22 the terms cannot cancel across ranks:
# E >= 1 gives at least 2^46 - 2^44 - 2^21 > 0, E <= -1 the opposite sign, and E = 0 leaves -S dy + dx, whose sign is that of
# -dy unless dy = 0, then that of dx: a first-order nudge to +x decides, the second-order one to +y breaks its ties.
S = 1 << 23
NEAR = Fraction(1, 1 << 20)         # a pixel may be left out only where the exact z + 1/2 lies this near an integer
HALF = Fraction(1, 2)


def second_statement(c, cs):
    """(depth, mask, skipped) of a case by the second statement: lists [frame][y][x]; skipped holds the pixels where some covering
    triangle's exact z + 1/2 is within NEAR of an integer."""
    n, w, h = c["n"], c["w"], c["h"]
    best = {}
    skipped = set()
    for r in cs["records"]:
        x, y = r["x"], r["y"]
        z = [Fraction(v) if np.isfinite(v) else None for v in r["z"]]
        inv = [Fraction(0) if v is None else 1 / v for v in z]
        flat = z[0] is not None and z[0] == z[1] == z[2]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        sg = 1 if area > 0 else -1
        edges = [(x[a], y[a], sg * (x[b] - x[a]), sg * (y[b] - y[a])) for a, b in ((1, 2), (2, 0), (0, 1))]
        # every pixel whose centre could be inside: the bounding box widened by a pixel, cut to the frame
        for py in range(max(min(y) // 16 - 1, 0), min(max(y) // 16 + 1, h - 1) + 1):
            cyy = 16 * py + 8
            for px in range(max(min(x) // 16 - 1, 0), min(max(x) // 16 + 1, w - 1) + 1):
                cxx = 16 * px + 8
                e = [dx * (cyy - ay) - dy * (cxx - ax) for ax, ay, dx, dy in edges]
                if not all(S * S * ev - S * dy + dx > 0 for ev, (_, _, dx, dy) in zip(e, edges)):
                    continue
                if flat:
                    zz = z[0] + HALF                 # (area / sum(e_i / z) = z: the e_i sum to the area)
                else:
                    zz = Fraction(sum(e)) / (e[0] * inv[0] + e[1] * inv[1] + e[2] * inv[2]) + HALF
                if abs(zz - round(zz)) < NEAR and zz < 65537:
                    skipped.add((r["frame"], py, px))
                d = 1 if zz < 1 else 65535 if zz >= 65535 else zz.numerator // zz.denominator
                key = 2 * d + (0 if r["head"] else 1)
                k = (r["frame"], py, px)
                if key < best.get(k, 1 << 40):
                    best[k] = key
    return best, skipped


@pytest.mark.parametrize("label", rf.LABELS)
def test_family_reaches_its_edge_and_the_restatement_holds(label):
    c = rf.all_cases()[label]
    cs = rf.census(c)
    c["reach"](cs)
    if c["scene"] != label:
        return                                       # (the geometry of this case is held under its scene's label)
    best, skipped = second_statement(c, cs)
    keys = rf.expected_keys(c)
    covered = np.argwhere(keys != rr.EMPTY)
    assert len(covered) == len(best) == int((cs["cover"] > 0).sum()), (len(covered), len(best))
    for f, y, x in covered.tolist():
        assert (f, y, x) in best, ("covered in render_ref only", f, y, x)
        if (f, y, x) not in skipped:
            assert int(keys[f, y, x]) == best[(f, y, x)], ("depth / mask", f, y, x, int(keys[f, y, x]), best[(f, y, x)])
    assert len(skipped) * 100 <= len(best), (len(skipped), len(best))


def test_sensor_cases_share_their_scene():
    cases = rf.all_cases()
    for label, c in cases.items():
        assert c["scene"] in cases and (c["scene"] == label or c["sensor"])
        s = cases[c["scene"]]
        assert (s["n"], s["w"], s["h"], len(s["instances"])) == (c["n"], c["w"], c["h"], len(c["instances"]))
