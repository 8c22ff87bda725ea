"""The grid-stride loop of the subject trackers' score kernels -- k_subject_track_score and k_rig_subject_score<STAGED> -- held to many
trips of mixed kinds (tests/score_trip_scenes.py).  Every other identification kernel runs one workgroup per
pair; these two run a fixed grid of G workgroups, each walking the pairs b, b + G, b + 2 G, ... of the step's want list and staging a
model into the same LDS on every trip, and the existing two-trip tests give every trip of a workgroup the same subject (64
candidates, G = 512).  Here the gallery size is chosen from the grid the tracker reports so that a workgroup's subject changes on
every trip, and the enrolled mask places the orders: run -> run with two different models, run -> skip -> run, everybody enrolled
with a partial last round, short refits (FEW_POINTS at the first pass) among full ones, a mask that shrinks from everybody to two
to one, streamed models of 1 025 points, the _device form between guard bands, and for the rig tracker a rig of 34 cameras whose
people are seen through bits 31, 32 and 33 of the view mask.  Every case on SubjectFitTracker and on RigSubjectFitTracker; every byte
of every record and of the state after every step against the restatements -- no tolerance.  The preconditions are computed from
the trip table with the G that info() reports and asserted; test_score_trip_scenes.py holds the same with G = 512 without a GPU."""
import contextlib

import numpy as np
import pytest

import fit_track_scenes as fts
import ident_ref as ir
import score_trip_scenes as ssc
import subject_track_gpu as stg
import subject_track_scenes as sts
import tracker_wave_scenes as tws
from depthhead_amd import _lib, fit, tracking
from gpu_kit import guarded, same_records, to_device, untouched

pytestmark = pytest.mark.gpu

KINDS = ("camera", "rig")
MANY = {"camera": 130, "rig": 9}                  # three update waves of wanting units: 64 + 64 + 2 cameras, 64 + 64 + 16 slots
PER_UNIT = {"camera": 1, "rig": ssc.SLOTS}
REC = {"camera": _lib.SUBJECT_TRACK_RECORD_DTYPE, "rig": _lib.RIG_SUBJECT_RECORD_DTYPE}
UNKNOWN = ir.UNKNOWN
NOBODY_BINDS = dict(retry=0, max_tries=0)


@pytest.fixture(scope="module")
def angles():
    return fit.angles()


@pytest.fixture(scope="module")
def grid():
    """(G, S): the score grid of a tracker with more pairs than workgroups, and the gallery size chosen for it.  Every case
    asserts that its own tracker reports this G."""
    import torch
    G = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    return G, ssc.choose_subjects(G)


@contextlib.contextmanager
def rig_trackers(angles, name, S, s, enrolled, ident, count):
    """`count` RigSubjectFitTrackers over the rigs of scene s and the gallery `name` of S subjects."""
    Rm = np.transpose(np.asarray(s.V, np.float64), (0, 2, 1))                     # the camera-to-world R, t a rig table takes
    tw = -np.einsum("nij,nj->ni", Rm, np.asarray(s.u, np.float64))
    with contextlib.ExitStack() as stack:
        got, _ = stack.enter_context(stg.gpu_set(name, S))
        cams = stack.enter_context(tracking.Cameras(s.Ks))
        rig = stack.enter_context(tracking.Rig(cams, Rm.astype(np.float32), tw.astype(np.float32), s.rig_begin))
        views = stack.enter_context(fit.Views(cams, s.V, s.u))
        model = stack.enter_context(fit.Model(*sts.generic(name)))
        yield [stack.enter_context(fit.RigSubjectFitTracker(rig, views, got, model, s.w, s.h, params=fit.rig_fit_track_params(**ssc.TRACK),
                                                            ident_params=fit.ident_views_params(**ssc.IDENT[ident]),
                                                            subject_params=fit.subject_track_params(**NOBODY_BINDS), enrolled=enrolled))
               for _ in range(count)]


@contextlib.contextmanager
def trackers(kind, angles, name, S, units, enrolled, ident="never", count=1):
    """`count` trackers of `kind` over the first `units` cameras or rigs of the scene; nobody retries later and no try is the last."""
    enrolled = None if enrolled is None else list(enrolled)
    if kind == "camera":
        with stg.pair(angles, name, S, ssc.cam_scene(name, S, units)[1], ssc.W, ssc.H, enrolled=enrolled, sub=NOBODY_BINDS, track=ssc.TRACK,
                      ident=ssc.IDENT[ident], trackers=count) as (trs, *_):
            yield trs if count > 1 else [trs]
    else:
        with rig_trackers(angles, name, S, ssc.rig_scene(name, S, units), enrolled, ident, count) as trs:
            yield trs


def inputs(kind, name, S, units, k):
    """The host arrays of step k in the order of the step call."""
    if kind == "camera":
        frames, _, poses = ssc.cam_scene(name, S, units)
        return frames[k], poses[k], fts.good_support(units)
    s = ssc.rig_scene(name, S, units)
    return (s.frames[k],) + tuple(s.inputs(ssc.rig_items(s, k)))


def step(kind, tr, args):
    prm = fit.fit_params(**ssc.FIT)
    return tr.step_poses(*args, None, prm) if kind == "camera" else tr.step_persons(*args, fit_params=prm)


def run_case(kind, angles, grid, name, units, masks, ident="never"):
    """The steps of `masks` on a fresh tracker beside the restated run, every record and the state compared; -> the run.  masks:
    per step the enrolled subjects, None: everybody."""
    G, S = grid
    masks = tuple(ssc.mask(S, m) for m in masks)
    run = ssc.run(kind, name, S, units, masks, ident, tws.angles_key(angles))
    with trackers(kind, angles, name, S, units, masks[0], ident) as (tr,):
        assert tr.info() == (units, S, G)
        for k, m in enumerate(masks):
            tr.set_enrolled(list(m))
            same_records(tr.state(), run.placed[k], f"state before step {k}")
            same_records(step(kind, tr, inputs(kind, name, S, units, k)), run.records[k], f"records of step {k}")
            same_records(tr.state(), run.state[k], f"state after step {k}")
    return run


def flat(run):
    return run.records.reshape(len(run.records), -1)


@pytest.mark.parametrize("kind", KINDS)
def test_run_then_run_with_different_models(kind, angles, grid):
    """Two subjects enrolled, G mod S apart: a workgroup that scores the first goes on to the second on its next trip, with the
    other model staged over the LDS it has just read.  Both scores of every unit are in its record as best and second."""
    G, S = grid
    units, pair = MANY[kind], ssc.two(G, S, 1)
    L = ssc.entries(kind, units)
    table = ssc.trips(G, S, L)
    assert L > 2 * ssc.WAVE and max(ssc.trip_counts(table)) >= 3 and ssc.subjects_in_a_row(table, ssc.mask(S, pair), "rr") > 0
    rec = flat(run_case(kind, angles, grid, ssc.NAME, units, (pair, pair)))
    assert (rec["identified"] == 1).all() and (rec["ident"]["eligible"] == 2).all() and (rec["subject"] == UNKNOWN).all()
    assert all({int(r["ident"]["best"]), int(r["ident"]["second"])} == set(pair) for r in rec.reshape(-1))


@pytest.mark.parametrize("kind", KINDS)
def test_run_skip_run(kind, angles, grid):
    """The two subjects 2 (G mod S) apart: between a workgroup's two runs lies a trip whose subject is not enrolled -- lane 0's zero
    record and the closing barrier alone."""
    G, S = grid
    units, pair = MANY[kind], ssc.two(G, S, 2)
    table = ssc.trips(G, S, ssc.entries(kind, units))
    assert ssc.subjects_in_a_row(table, ssc.mask(S, pair), "rsr") > 0 and ssc.subjects_in_a_row(table, ssc.mask(S, pair), "rr") == 0
    rec = flat(run_case(kind, angles, grid, ssc.NAME, units, (pair, pair)))
    assert (rec["identified"] == 1).all() and (rec["ident"]["eligible"] == 2).all()
    assert all({int(r["ident"]["best"]), int(r["ident"]["second"])} == set(pair) for r in rec.reshape(-1))


@pytest.mark.parametrize("kind", KINDS)
def test_everybody_enrolled_and_then_the_mask_shrinks(kind, angles, grid):
    """One update wave of units whose L S pairs are no multiple of G: workgroups of k and of k + 1 full trips, k >= 3, each with a
    different model on every trip.  Then the mask shrinks to two subjects and to one while every unit goes on wanting: a pair
    scored at one step and not enrolled at the next must have its score overwritten by the zero record, or the decision counts
    it -- eligible drops from S to 2 to 1."""
    G, S = grid
    units, L = ssc.one_wave_units(G, S, PER_UNIT[kind])
    table, k = ssc.trips(G, S, L), L * S // G
    assert (L * S) % G != 0 and k >= 3 and ssc.trip_counts(table) == [k, k + 1]
    assert all(len({s for _, s in t}) >= 2 for t in table)
    pair = ssc.two(G, S, 1)
    rec = flat(run_case(kind, angles, grid, ssc.NAME, units, (None, pair, pair[:1]), "far"))
    assert rec.shape[1] == L and (rec["identified"] == 1).all() and (rec["subject"] == UNKNOWN).all()
    assert [np.unique(r["ident"]["eligible"]).tolist() for r in rec] == [[S], [2], [1]]


@pytest.mark.parametrize("kind", KINDS)
def test_short_refits_among_full_ones(kind, angles, grid):
    """Everybody enrolled under a gate of 4 mm: about half the pairs end FEW_POINTS at their first pass and half run, so workgroups
    go from a short trip to a full one and back.  One update wave with everybody wanting: list entry e is unit e."""
    G, S = grid
    units, L = ssc.one_wave_units(G, S, PER_UNIT[kind])
    kind_of, table = ssc.kinds(kind, S, units, tws.angles_key(angles)), ssc.trips(G, S, L)
    short, full = int((kind_of == ssc.SHORT).sum()), int((kind_of == ssc.FULL).sum())
    print(kind, short, full)
    assert min(short, full) * 10 >= L * S
    assert ssc.kinds_in_a_row(table, kind_of, ssc.SHORT, ssc.FULL) > 0 and ssc.kinds_in_a_row(table, kind_of, ssc.FULL, ssc.SHORT) > 0
    rec = flat(run_case(kind, angles, grid, ssc.NAME, units, (None,), "gate"))
    assert (rec["identified"] == 1).all() and 0 < rec["ident"]["eligible"].max() < S


@pytest.mark.parametrize("kind", KINDS)
def test_streamed_models_with_a_sparse_mask(kind, angles, grid):
    """1 025 points, one more than are staged: the camera kernel's streamed branch and the rig kernel's STAGED = false instance, three
    trips and more of every workgroup with the two subjects of the first case enrolled."""
    G, S = grid
    units, L = ssc.one_wave_units(G, S, PER_UNIT[kind])
    pair = ssc.two(G, S, 1)
    table = ssc.trips(G, S, L)
    assert len(sts.mesh(ssc.STREAMED)[0]) == 1025 and min(ssc.trip_counts(table)) >= 3 and 2 * L <= 600
    assert ssc.subjects_in_a_row(table, ssc.mask(S, pair), "rr") > 0
    rec = flat(run_case(kind, angles, grid, ssc.STREAMED, units, (pair, pair)))
    assert (rec["identified"] == 1).all() and (rec["ident"]["eligible"] == 2).all()


@pytest.mark.parametrize("kind", KINDS)
def test_device_form_between_guard_bands(kind, angles, grid):
    """Step 0 of the first case as a _device step on a side stream, its records between guard bands, against the host form of a
    twin tracker and against the restatement."""
    import torch
    G, S = grid
    units, m = MANY[kind], ssc.mask(S, ssc.two(G, S, 1))
    run = ssc.run(kind, ssc.NAME, S, units, (m, m), "never", tws.angles_key(angles))
    args = inputs(kind, ssc.NAME, S, units, 0)
    nbytes = ssc.entries(kind, units) * REC[kind].itemsize
    stream = torch.cuda.Stream()
    with trackers(kind, angles, ssc.NAME, S, units, m, count=2) as (th, td):
        assert th.info() == td.info() == (units, S, G)
        want = step(kind, th, args)
        d = [to_device(a) for a in args]
        rec, rec_p, rec_o = guarded(nbytes, 8)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            extra = {} if kind == "camera" else {"max_heads": args[2].shape[1]}
            td.step_device(*(a.data_ptr() for a in d), rec_p, fit_params=fit.fit_params(**ssc.FIT), stream=stream.cuda_stream, **extra)
        stream.synchronize()
        assert untouched(rec, rec_o, nbytes)
        got = rec.cpu().numpy()[rec_o:rec_o + nbytes].view(REC[kind])
        same_records(got, want, "records of the _device step against the host form")
        same_records(got, run.records[0], "records of the _device step against the restatement")
        same_records(td.state(), th.state(), "state")
        same_records(td.state(), run.state[0], "state against the restatement")


def test_a_rig_of_34_cameras_seen_through_the_high_word_of_the_view_mask(angles):
    """One person seen by the cameras 0, 31, 32 and 33 of a rig of 34, another by camera 33 alone: the fit and the identification
    rebuild the 64-bit view mask, and camera 33's points are all the second person has.  Step 1 is a carried fit with the bound
    subject's model."""
    s = ssc.wide_scene()
    run = ssc.wide_run(tws.angles_key(angles))
    with rig_trackers(angles, ssc.NAME, ssc.WIDE_S, s, None, "binds", 1) as (tr,):
        assert tr.info()[:2] == (1, ssc.WIDE_S)
        for k in range(2):
            got = tr.step_persons(s.frames[k], *s.inputs(ssc.wide_items(s, k)), fit_params=fit.fit_params(**ssc.FIT))
            same_records(got, run.records[k], f"records of step {k}")
            same_records(tr.state(), run.state[k], f"state after step {k}")
            assert got[0, :2]["track"]["fit"]["views_used"].tolist() == list(ssc.WIDE_VIEWS)
            assert got[0, :2]["track"]["instance"]["views"].tolist() == list(ssc.WIDE_VIEWS)
            assert got[0, :2]["identified"].tolist() == ([1, 1] if k == 0 else [0, 0])
            if k == 0:
                assert (got[0, :2]["ident"]["status"] == ir.OK).all() and (got[0, :2]["ident"]["eligible"] == ssc.WIDE_S).all()
                assert (got[0, :2]["ident"]["points_best"] >= 24).all()
                bound = got[0, :2]["subject"].tolist()
            else:
                assert got[0, :2]["model"].tolist() == bound
