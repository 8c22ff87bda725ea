"""The restatement of the surface step (tests/surface_ref.py) by itself, on the CPU: what it must do on scenes
whose answer is known, and the evaluation -- head_mesh(3) with seeded bumps outside head_basis's span, eight poses, 320x240, noise
2, holes 0.02, six rounds of the restated driver.  The test asserts the evaluation on each of the three subjects; `python
tests/test_surface_ref.py` prints their table (DESIGN.md section 26 records it)."""
import functools

import numpy as np
import pytest

import fit_ref as fr
import shape_ref as sr
import subjects_ref as sb
import surface_ref as su
import surface_scenes as us
from depthhead_amd import synth

W, H = 160, 120


@functools.lru_cache(maxsize=None)
def head():
    v, t = synth.head_mesh(2)
    return v, t, synth.head_basis(v)


def bump_scene(n_frames=8, height=7.0, seed=5):
    """(the set, frames, K, instances at the true poses, the bump [n]): one subject whose only difference is a bump on its face."""
    v, t, B = head()
    st = su.Set(v, t, B, 1, max_offset=16.0)
    centre = int(np.argmin(st.nb[:, 2] + 0.002 * np.abs(v[:, 0]) + 0.002 * np.abs(v[:, 1] - 20.0)))    # faces the camera, off the nose
    disp = us.bump(v, centre, height, 30.0)
    frames, K, inst = us.splat_scene(v, st.nb, disp, W, H, n_frames, seed)
    return st, frames, K, inst, disp


def test_zero_offsets_are_section_25s_points_and_the_bound_grows_by_the_offsets():
    v, t, B = head()
    st = su.Set(v, t, B, 2, max_offset=12.0)
    c = np.array([[0.1, -0.2, 0.05, 0.3], [0.0, 0.0, 0.0, 0.0]])
    st.set_coeffs(c)
    for s in range(2):
        assert st.pts[s].tobytes() == sb.points(v, B, c[s]).tobytes()
    plain = sb.Set(v, t, B, 2)
    plain.set_coeffs(c)
    assert st.nrm.tobytes() == plain.nrm.tobytes() and st.nb.tobytes() == sb.normals(v, t)[0].tobytes()
    assert st.radius == plain.radius + 12.0 * 1.01
    o = np.where(np.arange(len(v)) % 2 == 0, 12.0, -12.0)
    st.set_offsets(0, o)
    assert np.sqrt((st.pts[0].astype(np.float64) ** 2).sum(axis=1)).max() <= st.radius * (1 + 1.2e-7)
    begin, lst = st.nbr
    assert begin[-1] == len(lst) == 2 * (len(v) + len(t) - 2) and (begin[1:] - begin[:-1]).min() >= 5        # a closed surface: 2 E entries
    for i in (0, 17, len(v) - 1):
        mine = lst[begin[i]:begin[i + 1]]
        assert (np.diff(mine) > 0).all() and i not in mine
        assert set(mine) == {int(x) for tri in t if i in tri for x in tri} - {i}


def test_a_bump_moves_its_observed_vertices_toward_it_and_a_subject_equal_to_the_model_moves_little():
    st, frames, K, inst, disp = bump_scene()
    rec = su.surface_step(frames, K, st, inst)[0]
    assert rec["status"] == su.OK and rec["instances"] == 8 and rec["rejected"] == 0 and rec["clamped"] == 0
    on_bump = np.flatnonzero((disp >= 3.0) & (st.counts[0] >= 4))
    assert len(on_bump) >= 5
    assert (np.abs(st.offsets[0][on_bump] - disp[on_bump]) < np.abs(disp[on_bump])).all()       # each strictly closer than it started
    assert (st.offsets[0][on_bump] > 0).all()
    assert rec["max_abs"] == np.abs(st.offsets[0]).max() and rec["observed"] == int((st.counts[0] >= 2).sum())
    # equal to the model: what is left is the sensor's noise (+-2 mm and the rounding to whole mm), smoothed
    v, t, B = head()
    flat = su.Set(v, t, B, 1, max_offset=16.0)
    frames0, K0, inst0 = us.splat_scene(v, flat.nb, np.zeros(len(v)), W, H, 8, 5)
    rec0 = su.surface_step(frames0, K0, flat, inst0)[0]
    print(f"bump: largest offset {rec['max_abs']:.3f} mm; no bump: largest {rec0['max_abs']:.3f} mm, mean |o| {np.abs(flat.offsets[0]).mean():.3f} mm")
    # a bound from the noise alone: one sample is off by at most 2.5 mm; a vertex seen once could move that far, no further
    assert rec0["status"] == su.OK and rec0["max_abs"] <= 2.5 and np.abs(flat.offsets[0]).mean() < 0.5 * np.abs(st.offsets[0][on_bump]).mean()


def test_an_empty_frame_gives_few_points_and_leaves_the_offsets():
    st, frames, K, inst, disp = bump_scene(n_frames=2)
    o = 0.25 * disp
    st.set_offsets(0, o)
    before = st.pts.copy()
    rec = su.surface_step(np.zeros_like(frames), K, st, inst)[0]
    assert rec["status"] == su.FEW_POINTS and rec["points"] == 0 and rec["instances"] == 0 and rec["observed"] == 0
    assert st.offsets[0].tobytes() == o.tobytes() and st.pts.tobytes() == before.tobytes() and rec["max_abs"] == np.abs(o).max()


def test_a_vertex_never_seen_gets_its_neighbours_jacobi_value():
    st, frames, K, inst, disp = bump_scene(n_frames=4)
    prm = su.params(iterations=1)
    start = 0.5 * disp
    st.set_offsets(0, start)
    su.surface_step(frames, K, st, inst, prm=prm)
    unseen = np.flatnonzero(st.counts[0] == 0)
    assert len(unseen) > 20                                                       # the back of the head
    begin, lst = st.nbr
    for i in unseen[:40]:
        s = np.float64(0.0)
        for j in lst[begin[i]:begin[i + 1]]:
            s = s + start[j]
        deg = np.float64(begin[i + 1] - begin[i])
        assert st.offsets[0][i] == (np.float64(0.0) + np.float64(0.5) * s) / ((np.float64(0.0) + np.float64(0.5) * deg) + np.float64(0.05))


def test_the_clamp_at_exactly_max_offset_and_one_ulp_beyond():
    """solve() on hand-made sums: mu = 0 and A = 1 make u_i = B_i / (1 + eps) -- so B is chosen to land on max_offset exactly, one
    ulp above and one ulp below, and the same three mirrored."""
    hi = 4.0
    eps = 0.25
    den = (np.float64(1.0) + np.float64(0.0) * np.float64(0.0)) + np.float64(eps)
    targets = [hi, np.nextafter(hi, 8.0), np.nextafter(hi, 0.0), -hi, -np.nextafter(hi, 8.0), -np.nextafter(hi, 0.0), np.inf, np.nan]
    nbr = (np.zeros(len(targets) + 1, np.int64), np.zeros(0, np.int64))
    # B_i / S must give u * den exactly: work in the fixed point's grid
    b = np.array([int(round(u * den * su.S)) if np.isfinite(u) else 0 for u in targets], np.int64)
    a = np.full(len(targets), int(su.S), np.int64)
    cnt = np.full(len(targets), 3, np.int64)
    o = np.zeros(len(targets))
    prm = su.params(mu=0.0, eps=eps, iterations=1)
    u, observed, clamped, rejected = su.solve(a, b, cnt, o, nbr, prm, hi)
    got = (b.astype(np.float64) / su.S) / den
    assert got[0] == hi and got[3] == -hi
    assert u[0] == hi and u[3] == -hi and observed == len(targets)
    want_clamped = int((np.abs(got[:6]) > hi).sum())
    assert clamped == want_clamped and (np.abs(u) <= hi).all()
    assert u[2] == got[2] and u[5] == got[5]                                       # below the limit: untouched
    # not finite: the old offset stays and is counted
    # not finite (an offset no device path can write, handed in directly): the old value stays and is counted, nothing else moves
    o2 = np.where(np.arange(len(targets)) == 6, np.inf, 1.5)
    u2, _, _, rejected2 = su.solve(a, b, cnt, o2, nbr, prm, hi)
    assert rejected2 == 1 and u2[6] == np.inf and np.isfinite(np.delete(u2, 6)).all()


def test_min_count_and_min_cos2_each_exclude_exactly_what_they_should():
    st, frames, K, inst, disp = bump_scene(n_frames=6)
    base = su.params(iterations=1, mu=0.0)
    su.surface_step(frames, K, st, inst, prm=base)
    counts, first = st.counts[0].copy(), st.offsets[0].copy()
    for mc in (1, 3, 5):
        again = su.Set(*head(), 1, max_offset=16.0)
        rec = su.surface_step(frames, K, again, inst, prm=dict(base, min_count=mc))[0]
        assert (again.counts[0] == counts).all() and rec["observed"] == int((counts >= mc).sum())
        assert (again.offsets[0][counts < mc] == 0.0).all()                       # mu = 0: no data, no movement
        assert (again.offsets[0][counts >= max(mc, 2)] == first[counts >= max(mc, 2)]).all()
    # min_cos2: the kept points are exactly those whose own squared cosine passes
    for m2 in (0.0, 0.5, 0.9):
        again = su.Set(*head(), 1, max_offset=16.0)
        rec = su.surface_step(frames, K, again, inst, prm=dict(base, min_cos2=m2))[0]
        total = 0
        for it in inst:
            ok0, _, _ = su.instance_terms(frames[it["frame"]], K, again.verts, again.nb, again.nb, it, dict(base, min_cos2=0.0))
            R, t = it["R"].astype(np.float64), it["t"].astype(np.float64)
            p = again.verts.astype(np.float64) @ R.T + t
            n = again.nb.astype(np.float64) @ R.T
            cos2 = ((n * p).sum(axis=1) ** 2) / (p * p).sum(axis=1)
            near = np.abs(cos2 - m2) < 1e-9                                         # (none sits on the threshold)
            assert not (ok0 & near).any()
            total += int((ok0 & (cos2 >= m2)).sum())
        assert rec["points"] == total
    assert su.surface_step(frames, K, su.Set(*head(), 1, max_offset=16.0), inst, prm=dict(base, min_cos2=0.9))[0]["points"] < \
        su.surface_step(frames, K, su.Set(*head(), 1, max_offset=16.0), inst, prm=dict(base, min_cos2=0.0))[0]["points"]


def test_two_subjects_in_one_call_equal_two_calls_and_skipped_instances_change_nothing():
    v, t, B = head()
    both = su.Set(v, t, B, 2, max_offset=16.0)
    scenes = [us.splat_scene(v, both.nb, us.bump(v, c, h, 25.0), W, H, 4, seed) for c, h, seed in ((3, 6.0, 7), (40, -5.0, 8))]
    frames = np.concatenate([s[0] for s in scenes])
    K = scenes[0][1]
    inst = scenes[0][2] + [dict(i, frame=i["frame"] + 4) for i in scenes[1][2]]
    who = [0] * 4 + [1] * 4
    rec = su.surface_step(frames, K, both, inst, who)
    for s in range(2):
        alone = su.Set(v, t, B, 1, max_offset=16.0)
        r1 = su.surface_step(frames, K, alone, [i for i, w in zip(inst, who) if w == s], [0] * 4)
        assert r1[0].tobytes() == rec[s].tobytes() and alone.offsets[0].tobytes() == both.offsets[s].tobytes()
        assert alone.pts[0].tobytes() == both.pts[s].tobytes() and alone.nrm[0].tobytes() == both.nrm[s].tobytes()
    # skipped and not-OK instances: as if they were not there
    more = su.Set(v, t, B, 2, max_offset=16.0)
    extra = inst + [dict(inst[0]), dict(inst[5]), dict(inst[6], frame=99), dict(inst[2], scale=np.float32(65.0))]
    who2 = who + [sr.SKIP, 1, 1, 0]
    status = [fr.OK] * 8 + [fr.OK, fr.FEW_POINTS, fr.OK, fr.OK]
    rec2 = su.surface_step(frames, K, more, extra, who2, 2, status)
    assert rec2.tobytes() == rec.tobytes() and more.offsets.tobytes() == both.offsets.tobytes()
    # fewer subjects than the set: subject 1 is left as it was
    part = su.Set(v, t, B, 2, max_offset=16.0)
    rec3 = su.surface_step(frames, K, part, inst, who, 1)
    assert len(rec3) == 1 and rec3[0].tobytes() == rec[0].tobytes() and not part.offsets[1].any()


# ---- the evaluation
def evaluate(seed, rounds=6):
    """Subject `seed`: the figures before (the generic model: round 1's fit) and after (the last round's fit with the refined
    model, the offsets after the last step): fit rms (mm), mean position error (mm), mean and worst surface error |o_i - true_i| (mm)
    over the vertices the last step observed at least 4 times."""
    v, t, _, B = us.eval_generic()
    frames, K, pos, Rs = us.eval_subject(seed)
    st = su.Set(v, t, B, 1, max_offset=16.0)
    _, _, _, trace = su.refine_subjects(frames, K, st, us.eval_starts(seed, pos, Rs), [0] * len(pos), rounds=rounds)
    true = us.eval_bumps(seed)
    seen = st.counts[0] >= 4

    def fit_figures(recs, inst):
        ok = [i for i, r in enumerate(recs) if r["status"] == fr.OK]
        e, n = sum(int(recs[i]["sum_r2_fixed"]) for i in ok), sum(int(recs[i]["points"]) for i in ok)
        err = [float(np.sqrt(((np.asarray(inst[i]["t"], np.float64) - pos[i]) ** 2).sum())) for i in ok]
        return float(np.sqrt(e / su.S / n)), float(np.mean(err))

    rms0, pos0 = fit_figures(trace[0][0], trace[0][2])
    rms1, pos1 = fit_figures(trace[-1][0], trace[-1][2])
    return {"rms": (rms0, rms1), "pos": (pos0, pos1), "mean": (float(np.abs(true[seen]).mean()), float(np.abs(st.offsets[0] - true)[seen].mean())),
            "worst": (float(np.abs(true[seen]).max()), float(np.abs(st.offsets[0] - true)[seen].max())), "seen": int(seen.sum())}


# twice the restatement's own worst "after" figure over the three seeds (the table in DESIGN.md section 26), as section 18 set its bounds
# measured (before -> after):   12: rms 1.81 -> 1.14, pos 1.63 -> 1.25, mean 0.81 -> 0.51, worst 7.11 -> 2.84
#                               13: rms 1.77 -> 1.24, pos 1.14 -> 0.70, mean 1.19 -> 0.42, worst 8.00 -> 1.34
#                               14: rms 1.63 -> 1.14, pos 1.04 -> 0.36, mean 0.87 -> 0.46, worst 7.91 -> 1.76
BOUND_RMS, BOUND_POS, BOUND_MEAN, BOUND_WORST = 2 * 1.24, 2 * 1.25, 2 * 0.51, 2 * 2.84


@pytest.mark.parametrize("seed", us.EVAL_SEEDS)
def test_the_evaluation(seed):
    r = evaluate(seed)
    print("subject %d: %s" % (seed, r))
    assert r["rms"][1] < r["rms"][0]
    assert r["rms"][1] <= BOUND_RMS and r["pos"][1] <= BOUND_POS and r["mean"][1] <= BOUND_MEAN and r["worst"][1] <= BOUND_WORST
    assert r["seen"] >= 100


if __name__ == "__main__":
    for seed in us.EVAL_SEEDS:
        r = evaluate(seed)
        print("subject %d: %d vertices seen >= 4 times; " % (seed, r["seen"]) +
              "; ".join("%s %.2f -> %.2f" % (k, r[k][0], r[k][1]) for k in ("rms", "pos", "mean", "worst")), flush=True)
