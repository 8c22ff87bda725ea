"""What test_gpu_tracker_waves.py assumes of tests/tracker_wave_scenes.py, held as facts of the restatements alone (DESIGN.md
sections 19 and 29): the want script's cameras want identification exactly as its table says, wave by wave; every fit in it is
accepted and every identification binds; under NEVER_BINDS nobody binds and everybody wants; the binding lifecycle's rows equal
the literals derived from the header's rules 2 and 3; the start kinds and the fit tracker's plans come out as arranged; and the
run of the first n cameras is the first n columns of the run of all of them.  No GPU."""
import numpy as np
import pytest

import fit_ref as fr
import fit_track_ref as ft
import fit_track_scenes as fts
import ident_ref as ir
import subject_track_ref as stf
import tracker_wave_scenes as tws

UNKNOWN = stf.UNKNOWN


def kinds(track):
    return (np.asarray(track["status"]) & 0xFF).tolist()


def test_the_scene_fills_waves_of_64_64_and_2_lanes():
    frames, Ks, poses = tws.scene()
    assert frames.shape == (tws.STEPS, 130, 48, 64) and Ks.shape == (130, 3, 3) and poses.shape == (tws.STEPS, 130)
    assert tws.who()[:7] == (tws.sts.STRANGER, 1, 2, 0, 1, tws.sts.STRANGER, 0) and len(tws.sts.mesh(tws.NAME)[0]) == 162
    assert [tws.per_wave(np.array(tws.wanting(k))) for k in range(5)] == list(tws.WANT_PER_WAVE)


def test_the_want_script_wants_what_its_table_says():
    run = tws.want_run()
    assert run.records.shape == (5, 130)
    for k in range(5):
        rec = run.records[k]
        assert rec["identified"].tolist() == tws.wanting(k), k
        assert tws.per_wave(rec["identified"]) == tws.WANT_PER_WAVE[k]
        assert kinds(rec["track"]) == [ft.FITTED if k == 0 else ft.CARRIED] * 130
        ran = rec["identified"] == 1
        assert (rec["ident"]["status"][ran] == ir.OK).all() and (rec["ident"]["status"][~ran] == ir.SKIPPED).all()
        assert (rec["subject"] < tws.S).all() and (run.state[k]["subject"] < tws.S).all()          # everyone is bound after every step
        assert (run.placed[k]["subject"] == UNKNOWN).tolist() == ([True] * 130 if k == 0 else [c in tws.UNBINDS[k] for c in range(130)])
    ran = run.records["identified"] == 1
    print(run.records["track"]["fit"]["points"].min(), run.records["ident"]["points_best"][ran].min())
    assert run.records["ident"]["points_best"][ran].min() >= 24                                   # min_points = 16 leaves room
    assert not run.state["wait"].any() and not run.state["tries"].any()


def test_the_first_cameras_of_the_run_are_the_run_of_the_first_cameras():
    """The rule is per camera: a fresh restated tracker of 65 cameras gives the first 65 columns of the run of 130."""
    fresh, cut = tws.want_run(None, 65, 3), tws.first_cameras(tws.want_run(), 65)
    for a, b in zip(fresh, cut):
        assert a.tobytes() == np.ascontiguousarray(b[:3]).tobytes()
    assert tws.unbinds(1, 65) == (64,) and tws.unbinds(2, 65) == (0, 63) and tws.unbinds(2, 63) == (0,) and tws.unbinds(1, 64) == ()


def test_under_never_binds_everybody_wants_at_every_step():
    run = tws.never_run()
    assert run.records.shape == (3, 65)
    assert (run.records["identified"] == 1).all() and (run.records["ident"]["status"] == ir.AMBIGUOUS).all()
    assert (run.records["subject"] == UNKNOWN).all() and run.records["tries"].tolist() == [[1] * 65, [2] * 65, [3] * 65]
    assert all(kinds(run.records[k]["track"]) == [ft.FITTED if k == 0 else ft.CARRIED] * 65 for k in range(3))


@pytest.mark.parametrize("retry,max_tries", sorted(tws.LIFECYCLE))
def test_the_lifecycle_rows_equal_the_literals_of_rules_2_and_3(retry, max_tries):
    run = tws.lifecycle_run(retry, max_tries)
    for c in range(tws.LIFECYCLE_CAMERAS):
        assert tws.lifecycle(run.records, run.state, c) == tws.LIFECYCLE[retry, max_tries], c
    assert (run.records["subject"] == UNKNOWN).all()
    if (retry, max_tries) == (0, 2):
        assert run.records["identified"][:, 0].tolist() == [1, 1, 0, 0, 0, 0]


def test_the_start_kinds_come_out_as_arranged_on_both_sides_of_the_boundaries():
    seen = tws.START_KINDS
    for kind in range(6):
        assert any(k == kind and c <= 63 for c, k in seen.items()) and any(k == kind and c >= 64 for c, k in seen.items()), kind
    assert {62, 63, 64, 65, 126, 127, 128, 129} <= set(seen)
    run = tws.start_kinds_run()
    rec = run.records[1]
    for c in range(130):
        status, identified = tws.START_ANSWER[seen.get(c, tws.CARRIED_BOUND)]
        assert (kinds(rec["track"])[c], int(rec["identified"][c])) == (status, identified), c
        if seen.get(c) == tws.DETECTED_BOUND:
            assert rec["model"][c] == tws.callers_subject(c) == rec["subject"][c]
        if seen.get(c) in (tws.CARRIED_UNBOUND, tws.DETECTED_UNBOUND):
            assert rec["model"][c] == UNKNOWN and rec["ident"]["status"][c] == ir.OK and rec["subject"][c] < tws.S


def test_the_fit_trackers_plans_come_out_as_arranged():
    want = tws.fit_kinds()
    for lo, hi in ((0, 64), (64, 128)):
        assert {want[1][c] for c in range(lo, hi)} == {ft.ABSENT, ft.NONE, ft.FITTED, ft.CARRIED, ft.REJECTED}
    assert {want[k][c] for k in range(3) for c in (128, 129)} == {ft.ABSENT, ft.NONE, ft.FITTED, ft.CARRIED, ft.REJECTED}
    run = tws.fit_run()
    assert [kinds(run.records[k]) for k in range(3)] == want
    rejected = (run.records["status"] & 0xFF) == ft.REJECTED
    assert (run.records["status"][rejected] == ft.REJECTED | ft.BAD_STATUS | ft.BAD_POINTS).all()
    # and the fresh run of 65 cameras is the first 65 columns
    frames, Ks, poses, sup, present = tws.fit_scene()
    tr = ft.Tracker(Ks[:65], *tws.sts.generic(tws.NAME), tws.ANGLES, prm=ft.params(**tws.TRACK))
    for k in range(2):
        got = tr.step(frames[k, :65], poses[k, :65], sup[k, :65], present[k, :65], fr.params(**tws.FIT))
        assert got.tobytes() == np.ascontiguousarray(run.records[k, :65]).tobytes() and tr.state.tobytes() == np.ascontiguousarray(run.state[k, :65]).tobytes()
    assert fts.good_support(1)["mass"][0] > 0
