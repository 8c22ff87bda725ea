"""What test_gpu_score_trips.py assumes of tests/score_trip_scenes.py, held as facts of the trip table and of the restatements
alone, with the grid of an MI355X, G = 512: the table against a brute-force enumeration -- G = 512 with S = 64
included, where every trip of a workgroup has the same subject, which is why the existing two-trip tests cannot see a stale model;
the gallery size chosen and the orders of trips each case places; who wants at every step of every scene; the kinds of the
short-refit case and their counts; the rig of 34 cameras; and a run of the first n units against the first n columns of the run of
all of them.  No GPU."""
import numpy as np
import pytest

import fit_ref as fr
import ident_ref as ir
import ident_views_ref as ivr
import score_trip_scenes as ssc

G = ssc.MI355X_GRID
S = ssc.choose_subjects(G)
UNKNOWN = ir.UNKNOWN
KINDS = ("camera", "rig")
MANY = {"camera": 130, "rig": 9}                  # units of three update waves: 64 + 64 + 2 cameras, 64 + 64 + 16 slots


def brute(G, S, L):
    """Every pair dealt to the workgroup that takes it, in order."""
    out = [[] for _ in range(G)]
    for pair in range(L * S):
        out[pair % G].append((pair // S, pair % S))
    return out


@pytest.mark.parametrize("G,S,L", [(512, 64, 9), (512, 65, 130), (512, 65, 24), (512, 63, 33), (8, 3, 7), (16, 5, 3), (608, 65, 144), (512, 65, 7)])
def test_the_trip_table_is_the_brute_force_enumeration(G, S, L):
    table = ssc.trips(G, S, L)
    assert table == brute(G, S, L)
    assert sorted(p for t in table for p in t) == [(e, s) for e in range(L) for s in range(S)]      # every pair once


def test_with_64_subjects_every_trip_of_a_workgroup_has_the_same_subject():
    """The existing tests' shape: 9 cameras, 64 candidates, 512 workgroups.  64 workgroups make a second trip, each with the
    subject of its first; a model staged on the first trip only would serve."""
    table = ssc.trips(512, 64, 9)
    assert ssc.trip_counts(table) == [1, 2] and sum(len(t) == 2 for t in table) == 64
    assert all(len({s for _, s in t}) == 1 for t in table)
    assert ssc.subjects_in_a_row(table, ssc.mask(64), "rr") == 0


def test_the_gallery_size_chosen_for_512_workgroups():
    assert (S, G % S) == (65, 57) and ssc.choose_subjects(608) == 65 and ssc.choose_subjects(520) == 63
    assert ssc.two(G, S, 1) == (2, 59) and ssc.two(G, S, 2) == (2, 51)
    assert ssc.one_wave_units(G, S, 1) == (24, 24) and ssc.one_wave_units(G, S, ssc.SLOTS) == (2, 32)
    with pytest.raises(AssertionError):
        ssc.choose_subjects(65 * 63 * 61 * 67)


@pytest.mark.parametrize("kind", KINDS)
def test_the_orders_of_trips_the_masks_place(kind):
    """Cases 1 and 2: two subjects one and two trips apart, three update waves of wanting units."""
    L = ssc.entries(kind, MANY[kind])
    assert L > 2 * ssc.WAVE
    table = ssc.trips(G, S, L)
    assert min(ssc.trip_counts(table)) >= 3
    near, far = ssc.mask(S, ssc.two(G, S, 1)), ssc.mask(S, ssc.two(G, S, 2))
    assert sum(near) == sum(far) == 2
    print(kind, ssc.trip_counts(table), ssc.subjects_in_a_row(table, near, "rr"), ssc.subjects_in_a_row(table, far, "rsr"))
    assert ssc.subjects_in_a_row(table, near, "rr") >= L // 2 and ssc.subjects_in_a_row(table, near, "rsr") == 0
    assert ssc.subjects_in_a_row(table, far, "rsr") >= L // 2 and ssc.subjects_in_a_row(table, far, "rr") == 0
    assert ssc.subjects_in_a_row(table, near, "sr") > 0 and ssc.subjects_in_a_row(table, near, "rs") > 0


@pytest.mark.parametrize("kind", KINDS)
def test_everybody_enrolled_in_one_update_wave(kind):
    """Case 3: workgroups of k and of k + 1 trips, k >= 3, and no workgroup sees one subject only."""
    units, L = ssc.one_wave_units(G, S, 1 if kind == "camera" else ssc.SLOTS)
    table = ssc.trips(G, S, L)
    k = L * S // G
    assert L <= ssc.WAVE and (L * S) % G != 0 and k >= 3 and ssc.trip_counts(table) == [k, k + 1]
    assert all(len({s for _, s in t}) == len(t) for t in table)                               # all of a workgroup's subjects differ


@pytest.mark.parametrize("kind", KINDS)
def test_two_enrolled_subjects_over_three_waves_of_wanting_units(kind):
    units = MANY[kind]
    for apart in (1, 2):
        m = ssc.mask(S, ssc.two(G, S, apart))
        run = ssc.run(kind, ssc.NAME, S, units, (m, m))
        rec = run.records.reshape(2, -1)
        assert rec.shape[1] == ssc.entries(kind, units)
        assert (rec["identified"] == 1).all() and (rec["ident"]["status"] == ir.AMBIGUOUS).all() and (rec["ident"]["eligible"] == 2).all()
        # both scores of every unit are in its record: best and second are the two enrolled subjects
        assert all({int(r["ident"]["best"]), int(r["ident"]["second"])} == set(ssc.two(G, S, apart)) for r in rec.reshape(-1))
        assert (rec["subject"] == UNKNOWN).all() and rec["tries"].tolist() == [[1] * rec.shape[1], [2] * rec.shape[1]]
        assert (rec["ident"]["points_best"] >= 24).all() and (rec["ident"]["points_second"] >= 24).all()      # min_points = 16 leaves room
    if kind == "rig":                                                                         # every slot of a rig has a fit of its own
        assert all(len({x.tobytes() for x in rig["track"]["instance"]}) == ssc.SLOTS for rig in run.records[0])


@pytest.mark.parametrize("kind", KINDS)
def test_the_mask_shrinks_and_nobody_binds(kind):
    """Cases 3 and 5: everybody, then the two of case 1, then one of them; every unit wants at every step."""
    units, L = ssc.one_wave_units(G, S, 1 if kind == "camera" else ssc.SLOTS)
    pair = ssc.two(G, S, 1)
    run = ssc.run(kind, ssc.NAME, S, units, (ssc.mask(S), ssc.mask(S, pair), ssc.mask(S, pair[:1])), "far")
    rec = run.records.reshape(3, -1)
    assert rec.shape[1] == L and (rec["identified"] == 1).all() and (rec["ident"]["status"] == ir.FAR).all()
    assert [np.unique(r["ident"]["eligible"]).tolist() for r in rec] == [[S], [2], [1]]
    assert (rec["subject"] == UNKNOWN).all() and (run.state["subject"] == UNKNOWN).all()
    assert (rec[2]["ident"]["best"] == pair[0]).all() and (rec[2]["ident"]["second"] == UNKNOWN).all()
    # a score of step 0 left standing would be eligible at step 1: step 0's best is mostly neither of the two
    assert np.isin(rec[0]["ident"]["best"], pair, invert=True).sum() >= L // 2


@pytest.mark.parametrize("kind", KINDS)
def test_short_refits_among_full_ones(kind):
    """Case 4: the kinds under the gate written down in the scene module, their counts, and their orders within a workgroup."""
    units, L = ssc.one_wave_units(G, S, 1 if kind == "camera" else ssc.SLOTS)
    kind_of, table = ssc.kinds(kind, S, units), ssc.trips(G, S, L)
    short, full = int((kind_of == ssc.SHORT).sum()), int((kind_of == ssc.FULL).sum())
    counts = (short, full, ssc.kinds_in_a_row(table, kind_of, ssc.SHORT, ssc.FULL), ssc.kinds_in_a_row(table, kind_of, ssc.FULL, ssc.SHORT))
    print(kind, counts)
    assert counts == ssc.KIND_COUNTS[kind] and short + full == L * S
    assert min(short, full) * 10 >= L * S and counts[2] > 0 and counts[3] > 0
    who = ssc.cam_who(units, S) if kind == "camera" else [w for w in ssc.rig_who(units, S) for _ in range(ssc.SLOTS)]
    assert sum(kind_of[e, who[e]] == ssc.FULL for e in range(L)) >= L // 4                       # the subject in the frame runs
    # and the restated step's eligible counts are the full pairs with enough points: below S, above 0 somewhere
    rec = ssc.run(kind, ssc.NAME, S, units, (ssc.mask(S),), "gate").records[0].reshape(-1)
    assert (rec["ident"]["eligible"] <= (kind_of == ssc.FULL).sum(axis=1)).all() and 0 < rec["ident"]["eligible"].max() < S


@pytest.mark.parametrize("kind,units", [("camera", 24), ("rig", 2)])
def test_streamed_models_with_a_sparse_mask(kind, units):
    """Case 6: 1 025 points, the two subjects of case 1, at least three trips of every workgroup and at most 600 run pairs."""
    assert len(ssc.sts.mesh(ssc.STREAMED)[0]) == 1025 and ssc.one_wave_units(G, S, 1 if kind == "camera" else ssc.SLOTS)[0] == units
    m = ssc.mask(S, ssc.two(G, S, 1))
    rec = ssc.run(kind, ssc.STREAMED, S, units, (m, m)).records.reshape(2, -1)
    assert (rec["identified"] == 1).all() and (rec["ident"]["eligible"] == 2).all() and 2 * rec.shape[1] <= 600
    assert min(ssc.trip_counts(ssc.trips(G, S, rec.shape[1]))) >= 3


def test_the_rig_of_34_cameras():
    """Case 8: both people identified at step 0 over views at and above bit 32, and carried with the bound model at step 1."""
    s, run = ssc.wide_scene(), ssc.wide_run()
    assert s.n_cams == 34 and s.n_rigs == 1 and ssc.WIDE_VIEWS == (0x380000001, 0x200000000)
    rec = run.records[:, 0, :2]
    assert rec["identified"].tolist() == [[1, 1], [0, 0]] and (rec["ident"]["status"][0] == ir.OK).all() and (rec["ident"]["eligible"][0] == 3).all()
    assert rec["track"]["fit"]["views_used"].tolist() == [list(ssc.WIDE_VIEWS)] * 2
    assert rec["model"][1].tolist() == rec["subject"][0].tolist() and (rec["subject"][0] < 3).all()
    # the identification of person 0 counted the points of the cameras 32 and 33: over the low word's views alone it finds fewer
    t = rec[0, 0]["track"]["instance"]
    st, best = ssc.restated_set(ssc.NAME, 3), int(rec[0, 0]["ident"]["best"])
    low = {"first_cam": 0, "views": int(t["views"]) & 0xFFFFFFFF, "R": t["R"].reshape(3, 3), "t": t["t"], "scale": np.float32(t["scale"])}
    got = ivr.score(s.frames[0], s.Ks, s.V, s.u, st.pts[best], st.nrm[best], low, ir.params(**ssc.IDENT["binds"]))[2]
    assert got["status"] == fr.OK and 0 < got["points"] < rec[0, 0]["ident"]["points_best"]
    assert rec[0, 1]["ident"]["points_best"] >= 24                                            # person 1 has camera 33 alone


@pytest.mark.parametrize("kind,n", [("camera", 24), ("rig", 2)])
def test_the_first_units_of_the_run_are_the_run_of_the_first_units(kind, n):
    """The rule is per camera and per rig: a fresh run of the first n units is the first n columns of the run of all of them."""
    m = ssc.mask(S, ssc.two(G, S, 1))
    fresh, cut = ssc.run(kind, ssc.NAME, S, n, (m, m)), ssc.first_units(ssc.run(kind, ssc.NAME, S, MANY[kind], (m, m)), n)
    for a, b in zip(fresh, cut):
        assert a.tobytes() == np.ascontiguousarray(b).tobytes()
