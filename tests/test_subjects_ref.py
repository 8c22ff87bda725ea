"""The restatement of a subject set (tests/subjects_ref.py) held to what the project already has, without a
GPU: its update to fit.deform and fit.vertex_normals byte for byte, its driver to shape_ref.adapt, and the rule's edges -- the
clamp, increments that are not finite, records that are not OK, a mesh that deforms to a zero normal -- to their definition.

`python tests/test_subjects_ref.py` prints the table of DESIGN.md section 25: three subjects adapted together for six rounds
beside each adapted alone."""
import functools
import sys

import numpy as np
import pytest

import fit_ref as fr
import shape_ref as sr
import shape_scenes as ss
import subjects_ref as sb
import subjects_scenes as sc
from depthhead_amd import fit, synth
from subjects_scenes import H, VARIATIONS, W, collapsing_disc, fan_mesh, seeded_fields, three_subjects


@functools.lru_cache(maxsize=None)
def meshes():
    tetra = (np.array([(0, 0, 0), (40, 0, 0), (0, 40, 0), (0, 0, 40)], np.float32), np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.uint32))
    out = {"tetrahedron": tetra, "box": synth.box_mesh((-30.0, -20.0, -10.0), (30.0, 20.0, 10.0)), "head": synth.head_mesh(2), "fan": fan_mesh()}
    return {k: (v, t, seeded_fields(v, 4, 77 + i)) for i, (k, (v, t)) in enumerate(out.items())}


COEFFS = ((0.0, 0.0, 0.0, 0.0), (0.08, -0.07, 0.06, 0.0), (-0.5, 0.5, 0.25, -0.125), (0.3, 1e-9, -0.41, 0.07))


@pytest.mark.parametrize("name", ("tetrahedron", "box", "head", "fan"))
def test_the_update_is_deform_and_vertex_normals(name):
    v, t, B = meshes()[name]
    st = sb.Set(v, t, B, len(COEFFS))
    st.set_coeffs(COEFFS)
    for s, c in enumerate(COEFFS):
        want_v = fit.deform(v, B, c)
        assert st.pts[s].tobytes() == want_v.tobytes() == sr.deform(v, B, c).tobytes(), (name, s)
        assert st.nrm[s].tobytes() == fit.vertex_normals(want_v, t).tobytes(), (name, s)
        assert st.state["zero_normals"][s] == 0
    if name == "fan":
        begin, _ = st.lists
        assert begin[1] - begin[0] == 300 and (begin[2:] - begin[1:-1] == 2).all()


def test_corner_lists_are_the_corners_in_order():
    for name, (v, t, _) in meshes().items():
        begin, corners = sb.corner_lists(t, len(v))
        flat = t.reshape(-1)
        assert begin[0] == 0 and begin[-1] == len(flat) == len(corners)
        assert sorted(corners.tolist()) == list(range(len(flat)))
        for i in range(len(v)):
            run = corners[begin[i]:begin[i + 1]]
            assert (flat[run] == i).all() and (np.diff(run) > 0).all(), (name, i)
    # a vertex named twice by one triangle, and a vertex no triangle names
    begin, corners = sb.corner_lists(np.array([(0, 0, 1), (3, 1, 0)]), 4)
    assert begin.tolist() == [0, 3, 5, 5, 6] and corners.tolist() == [0, 1, 5, 2, 4, 3]
    twice = np.array([(0, 0, 0), (9, 0, 0), (0, 9, 0)], np.float32)
    n, zeros = sb.normals(twice, np.array([(0, 1, 2), (0, 0, 1)]))
    assert n.tobytes() == fit.vertex_normals(twice, np.array([(0, 1, 2), (0, 0, 1)])).tobytes() and zeros == 0


def record(delta, status=sr.OK):
    r = np.zeros((), sr.RECORD_DTYPE)
    r["delta"][:len(delta)] = delta
    r["status"] = status
    return r


def test_apply_the_clamp_at_max_coeff_and_one_ulp_beyond():
    hi = np.float64(0.5)
    st = np.zeros((), sb.STATE_DTYPE)
    st["coeffs"][:3] = (0.25, -0.25, 0.1)
    at = sb.apply(st, record([0.25, -0.25, 0.0]), 3, 0.5)
    assert at["coeffs"][:3].tolist() == [0.5, -0.5, 0.1] and at["flags"] == 0 and (at["applied"], at["rejected"]) == (1, 0)
    ulp = np.nextafter(hi, 1.0) - hi
    st["coeffs"][:3] = (0.5, -0.5, 0.1)
    beyond = sb.apply(st, record([ulp, 0.0, 0.0]), 3, 0.5)
    assert np.float64(0.5) + ulp > 0.5 and beyond["coeffs"][0] == 0.5 and beyond["flags"] == sb.CLAMPED and beyond["applied"] == 1
    below = sb.apply(st, record([0.0, -ulp, 0.0]), 3, 0.5)
    assert below["coeffs"][1] == -0.5 and below["flags"] == sb.CLAMPED
    inside = sb.apply(st, record([-ulp, ulp, 0.0]), 3, 0.5)
    assert inside["coeffs"][0] == hi - ulp < hi and inside["coeffs"][1] == -(hi - ulp) and inside["flags"] == 0
    far = sb.apply(st, record([1e308, -1e308, 1e308]), 3, 0.5)
    assert far["coeffs"][:3].tolist() == [0.5, -0.5, 0.5] and far["flags"] == sb.CLAMPED
    # a field beyond K is not the subject's: its delta is ignored, its coefficient stays 0
    two = sb.apply(st, record([0.0, 0.0, 7.0, np.nan]), 2, 0.5)
    assert two["coeffs"][:4].tolist() == [0.5, -0.5, 0.1, 0.0] and two["flags"] == 0 and two["applied"] == 1
    # the flag stays
    again = sb.apply(beyond, record([-0.25, 0.0, 0.0]), 3, 0.5)
    assert again["coeffs"][0] == 0.25 and again["flags"] == sb.CLAMPED and again["applied"] == 2


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_apply_rejects_an_increment_that_is_not_finite(bad):
    st = np.zeros((), sb.STATE_DTYPE)
    st["coeffs"][:3] = (0.25, -0.25, 0.1)
    for k in range(3):
        d = [0.125, 0.125, 0.125]
        d[k] = bad
        got = sb.apply(st, record(d), 3, 0.5)
        assert got["coeffs"].tobytes() == st["coeffs"].tobytes() and (got["applied"], got["rejected"], got["flags"]) == (0, 1, sb.NONFINITE)
    counted = np.zeros((), sb.STATE_DTYPE)
    counted["rejected"] = counted["applied"] = 0xFFFFFFFF
    assert sb.apply(counted, record([bad]), 1, 0.5)["rejected"] == 0xFFFFFFFF and sb.apply(counted, record([0.1]), 1, 0.5)["applied"] == 0xFFFFFFFF


@pytest.mark.parametrize("status", (sr.FEW_POINTS, sr.SINGULAR, 7))
def test_a_record_that_is_not_ok_applies_nothing(status):
    st = np.zeros((), sb.STATE_DTYPE)
    st["coeffs"][:2], st["flags"] = (0.25, -0.25), sb.CLAMPED
    got = sb.apply(st, record([0.125, np.nan], status), 2, 0.5)
    assert got.tobytes() == st.tobytes()
    # and the set still evaluates the subject: its model is that of its coefficients
    v, t, B = meshes()["box"]
    s = sb.Set(v, t, B, 2)
    s.update(np.array([record([0.1, 0.2, 0.3, 0.4]), record([0.1, 0.2, 0.3, 0.4], status)]))
    assert s.state["applied"].tolist() == [1, 0] and not s.state["coeffs"][1].any()
    assert s.pts[1].tobytes() == fit.deform(v, B, np.zeros(4)).tobytes() and s.pts[0].tobytes() == fit.deform(v, B, (0.1, 0.2, 0.3, 0.4)).tobytes()


def test_a_mesh_that_deforms_to_a_zero_normal():
    v, t, B, hub = collapsing_disc()
    st = sb.Set(v, t, B, 2)
    assert st.state["zero_normals"].tolist() == [0, 0] and (st.nrm[0][:, 2] < 0.0).all()          # the base mesh faces the camera
    st.set_coeffs([[0.25]], first=1)
    assert (st.pts[1][1:7] == v[hub]).all() and st.pts[1].tobytes() == fit.deform(v, B, [0.25]).tobytes()
    assert st.nrm[1].tobytes() == fit.vertex_normals(st.pts[1], t).tobytes()
    assert st.state["zero_normals"].tolist() == [0, 1] and not st.nrm[1][hub].any() and (np.abs(st.nrm[1][1:]).sum(axis=1) > 0.9).all()
    # the zero-normal vertex is never associated: the fit's pass over the model and over the model without it give the same sums
    K = synth.default_intrinsic(W, H)
    frame = np.full((H, W), 800, np.uint16)
    R, pos = np.eye(3), np.array([0.0, 0.0, 800.0])
    keep = np.arange(len(v)) != hub
    whole = fr.one_pass(frame, K, st.pts[1], st.nrm[1], np.float64(1.0), R, pos, 25.0)
    without = fr.one_pass(frame, K, st.pts[1][keep], st.nrm[1][keep], np.float64(1.0), R, pos, 25.0)
    assert whole == without and whole[3] == len(v) - 1
    assert fr.one_pass(frame, K, st.pts[0], st.nrm[0], np.float64(1.0), R, pos, 25.0)[3] == len(v)   # at the base it is


def same_instances(got, want, offset=0):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a["frame"] == b["frame"] + offset and a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes()


@pytest.mark.parametrize("seed", (12, 13))
def test_one_subject_is_shape_refs_adapt(seed):
    """S = 1 on section 20's scene: every coefficient, instance and record of every round equal to shape_ref.adapt's.  The two
    drivers differ where a coefficient meets the clamp, so the test needs seeds on which none comes near max_coeff = 0.5."""
    v, t, _, B = ss.generic()
    frames, K, pos, Rs = ss.subject(W, H, seed)
    starts = ss.rough_instances(seed, pos, Rs)
    want_c, want_inst, want_trace = sr.adapt(frames, K, v, t, B, starts, fit.vertex_normals)
    assert all(np.abs(c + rec["delta"][:4]).max() < 0.25 for c, _, rec in want_trace)              # the precondition
    state, inst, (recs, srec), trace = sb.adapt_subjects(frames, K, sb.Set(v, t, B, 1), starts, [0] * len(starts))
    assert state["coeffs"][0, :4].tobytes() == want_c.tobytes() and not state["coeffs"][0, 4:].any()
    assert (state["applied"][0], state["rejected"][0], state["flags"][0], state["zero_normals"][0]) == (6, 0, 0, 0)
    same_instances(inst, want_inst)
    assert len(trace) == len(want_trace) == 6
    for (c, fit_recs, shape_recs), (wc, wfit, wshape) in zip(trace, want_trace):
        assert c[0, :4].tobytes() == wc.tobytes() and fit_recs == wfit and shape_recs[0].tobytes() == wshape.tobytes()
    assert recs == want_trace[-1][1] and srec[0].tobytes() == want_trace[-1][2].tobytes()


def test_two_subjects_are_driven_apart_over_three_rounds():
    v, t, _, B = ss.generic()
    frames, K, starts, who = three_subjects()
    st = sb.Set(v, t, B, 2)
    state, inst, _, trace = sb.adapt_subjects(frames[:16], K, st, starts[:16], who[:16], rounds=3)
    assert not trace[0][0].any()                                                                    # both start at the base
    assert st.pts[0].tobytes() != st.pts[1].tobytes() and st.nrm[0].tobytes() != st.nrm[1].tobytes()
    for s in range(2):
        want_c, want_inst, _ = sc.alone(s, rounds=3)
        assert state["coeffs"][s, :4].tobytes() == want_c.tobytes()
        same_instances(inst[8 * s:8 * s + 8], want_inst, offset=8 * s)
        assert st.pts[s].tobytes() == fit.deform(v, B, want_c).tobytes()
    # apart: subject 0 is wider and shorter than subject 1
    assert state["coeffs"][0, 0] > state["coeffs"][1, 0] + 0.03 and state["coeffs"][0, 1] < state["coeffs"][1, 1] - 0.03


def rms_of(rec):
    return float(np.sqrt(int(rec["sum_r2_fixed"]) / sr.S / int(rec["points"])))


def test_three_subjects_adapted_together_are_each_adapted_alone():
    """The subjects do not interact: after six rounds each one's coefficients, instances, fit records and shape record (so its
    residual) are exactly those shape_ref.adapt reaches for it alone.  No accuracy bound is asserted here beyond that
    equality: section 20's tests hold the single subject's."""
    state, inst, (recs, srec), _ = sc.together()
    for s in range(3):
        want_c, want_inst, want_trace = sc.alone(s)
        assert state["coeffs"][s, :4].tobytes() == want_c.tobytes(), s
        same_instances(inst[8 * s:8 * s + 8], want_inst, offset=8 * s)
        assert recs[8 * s:8 * s + 8] == want_trace[-1][1]
        assert srec[s].tobytes() == want_trace[-1][2].tobytes()
    assert state["applied"].tolist() == [6, 6, 6] and not state["flags"].any() and not state["zero_normals"].any()


if __name__ == "__main__":
    state, inst, (recs, srec), _ = sc.together()
    print("| subject | true stretch | coefficients together | equal to alone | residual rms before the last step (mm) | alone |")
    for s in range(3):
        want_c, _, want_trace = sc.alone(s)
        print(f"| {s} | {list(VARIATIONS[s])} | {np.round(state['coeffs'][s, :4], 4).tolist()} | {state['coeffs'][s, :4].tobytes() == want_c.tobytes()} "
              f"| {rms_of(srec[s]):.3f} | {rms_of(want_trace[-1][2]):.3f} |")
    sys.exit(0)
