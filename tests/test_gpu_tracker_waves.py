"""The fit trackers' per-camera kernels with more than one wave of cameras (tests/tracker_wave_scenes.py; DESIGN.md sections 19 and
29): k_subject_track_seed / _update and k_fit_track_seed / _update run one lane per camera in workgroups of one wave, and every
other test gives them at most 15 cameras -- one workgroup, blockIdx.x == 0, the want list's base always 0.  Here 130 cameras fill
waves of 64, 64 and 2 lanes, and the want script places which of them want identification: all, one full wave between two empty
ones, the first lane, the last lane and the last camera, nobody after the list held three, alternate lanes.  Camera counts about
the wave (63, 64, 65, 128, 129); everybody wanting at every step; the binding lifecycle's four (retry, max_tries) rows; every start
kind on both sides of a wave boundary in one launch; the _device forms at 65 cameras between guard bands; and the plain fit tracker
at 64, 65 and 130 cameras with every record kind about the boundaries.  Every byte of every record and of the state against the
restatements, as test_gpu_subject_tracker.py and test_gpu_fit_tracker.py hold them -- no tolerance.  The preconditions (who wants,
who binds, which kinds come out) are facts of the restatement that test_tracker_wave_scenes.py checks without a GPU.
Not reached: the saturation of tries, bound_age and lost at 2^32 - 1 -- no call sets a state."""
import numpy as np
import pytest

import fit_track_ref as ft
import fit_track_scenes as fts
import subject_track_ref as stf
import subject_track_scenes as sts
import tracker_wave_scenes as tws
from depthhead_amd import _lib, fit, tracking
from gpu_kit import guarded, same_records, to_device, untouched
from subject_track_gpu import both, pair

pytestmark = pytest.mark.gpu

N, S, W, H = tws.N, tws.S, tws.W, tws.H
REC, FIT_REC = _lib.SUBJECT_TRACK_RECORD_DTYPE, _lib.FIT_TRACK_RECORD_DTYPE
UNKNOWN = stf.UNKNOWN


@pytest.fixture(scope="module")
def angles():
    return fit.angles()


def trackers(angles, n, ident="always", sub=(0, 0), count=1):
    """pair() over the first n cameras of the scene; the restated tracker it makes is left aside for a Replay of the cached run."""
    return pair(angles, tws.NAME, S, tws.scene()[1][:n], W, H, sub=dict(retry=sub[0], max_tries=sub[1]), track=tws.TRACK, ident=tws.IDENT[ident],
                trackers=count)


def kinds(track):
    return (np.asarray(track["status"]) & 0xFF).tolist()


def run_script(tr, run, n, steps, binds=True):
    """The steps of a script on `tr` beside the restated run, with the want script's binds before each; -> the GPU's records [steps, n]."""
    frames, _, poses = tws.scene()
    ref, sup, out = tws.Replay(run), fts.good_support(n), []
    for k in range(steps):
        for c in tws.unbinds(k, n) if binds else ():
            tr.bind(c, None)
        ref.placed(k)
        same_records(tr.state(), ref.state, f"state before step {k}")
        out.append(both(tr, ref, frames[k, :n], poses[k, :n], sup, what=f"step {k}", fit_kw=tws.FIT))
    return np.stack(out)


def test_want_script_130_cameras(angles):
    with trackers(angles, N) as (tr, *_):
        assert tr.info()[0] == N
        rec = run_script(tr, tws.want_run(tws.angles_key(angles)), N, len(tws.UNBINDS))
    for k in range(len(tws.UNBINDS)):
        assert rec["identified"][k].tolist() == tws.wanting(k) and tws.per_wave(rec["identified"][k]) == tws.WANT_PER_WAVE[k], k


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_camera_counts_about_the_wave(angles, n):
    run = tws.first_cameras(tws.want_run(tws.angles_key(angles)), n)
    with trackers(angles, n) as (tr, *_):
        assert tr.info()[0] == n
        rec = run_script(tr, run, n, 3)
    assert [r.tolist() for r in rec["identified"]] == [tws.wanting(k, n) for k in range(3)]


def test_everybody_wants_at_every_step_65_cameras(angles):
    run = tws.never_run(tws.angles_key(angles))
    with trackers(angles, 65, "never") as (tr, *_):
        rec = run_script(tr, run, 65, 3, binds=False)
        state = tr.state()
    assert (rec["identified"] == 1).all() and (rec["subject"] == UNKNOWN).all() and (state["subject"] == UNKNOWN).all()
    assert rec["tries"].tolist() == [[1] * 65, [2] * 65, [3] * 65] and state["tries"].tolist() == [3] * 65


@pytest.mark.parametrize("retry,max_tries", sorted(tws.LIFECYCLE))
def test_lifecycle_rows(angles, retry, max_tries):
    run = tws.lifecycle_run(retry, max_tries, tws.angles_key(angles))
    frames, _, poses = tws.scene()
    n = tws.LIFECYCLE_CAMERAS
    with trackers(angles, n, "never", (retry, max_tries)) as (tr, *_):
        ref, rec, state = tws.Replay(run), [], []
        for k in range(tws.STEPS):
            rec.append(both(tr, ref, frames[k, :n], poses[k, :n], fts.good_support(n), what=f"step {k}", fit_kw=tws.FIT))
            state.append(tr.state())
    rec, state = np.stack(rec), np.stack(state)
    for c in range(n):
        assert tws.lifecycle(rec, state, c) == tws.LIFECYCLE[retry, max_tries], c


def test_every_start_kind_on_both_sides_of_a_wave_boundary(angles):
    run = tws.start_kinds_run(tws.angles_key(angles))
    frames, _, poses = tws.scene()
    with trackers(angles, N) as (tr, *_):
        ref = tws.Replay(run)
        both(tr, ref, frames[0], poses[0], fts.good_support(N), what="step 0", fit_kw=tws.FIT)
        present, sup = tws.arrange_start_kinds(tr)
        ref.placed(1)
        same_records(tr.state(), ref.state, "state after the resets and the binds")
        rec = both(tr, ref, frames[1], poses[1], sup, present, what="step 1", fit_kw=tws.FIT)
    got = kinds(rec["track"])
    for c, kind in tws.START_KINDS.items():
        assert (got[c], int(rec["identified"][c])) == tws.START_ANSWER[kind], c
    assert all(got[c] == ft.CARRIED and rec["identified"][c] == 0 for c in range(N) if c not in tws.START_KINDS)


def test_device_form_65_cameras_between_guard_bands(angles):
    """Step 1 of 65 cameras -- camera 64 alone in the second wave; cameras 0, 63 and 64 want, camera 1 is absent -- as a _device step
    on a side stream against the host form of a twin tracker, its records between guard bands: a lane of the second wave past the
    cameras that wrote a record shows here."""
    import torch
    n = 65
    frames, _, poses = tws.scene()
    stream = torch.cuda.Stream()
    with trackers(angles, n, count=2) as ((th, td), *_):
        sup0 = fts.good_support(n)
        first = th.step_poses(frames[0, :n], poses[0, :n], sup0, None, fit.fit_params(**tws.FIT))
        same_records(td.step_poses(frames[0, :n], poses[0, :n], sup0, None, fit.fit_params(**tws.FIT)), first, "step 0 of the twin")
        for t in (th, td):
            t.bind(64, None); t.bind(63, None); t.reset(0)
        present = np.ones(n, np.uint8)
        present[1] = 0
        want = th.step_poses(frames[1, :n], poses[1, :n], sup0, present, fit.fit_params(**tws.FIT))
        d_in = [to_device(a) for a in (frames[1, :n], poses[1, :n], sup0, present)]
        rec, rec_p, rec_o = guarded(n * REC.itemsize, 8)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            td.step_device(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), rec_p, present_ptr=d_in[3].data_ptr(),
                           fit_params=fit.fit_params(**tws.FIT), stream=stream.cuda_stream)
        stream.synchronize()
        assert untouched(rec, rec_o, n * REC.itemsize)
        same_records(rec.cpu().numpy()[rec_o:rec_o + n * REC.itemsize].view(REC), want, "records of the _device step")
        same_records(td.state(), th.state(), "state")
    assert want["identified"].tolist() == [1] + [0] * 62 + [1, 1] and kinds(want["track"])[:2] == [ft.FITTED, ft.ABSENT]
    run = tws.first_cameras(tws.want_run(tws.angles_key(angles)), n)
    same_records(first, run.records[0], "step 0 against the restatement")


# ---- the plain fit tracker
def fit_pair(n):
    frames, Ks, poses, sup, present = tws.fit_scene()
    return tracking.Cameras(Ks[:n]), fit.Model(*sts.generic(tws.NAME)), (frames[:, :n], poses[:, :n], sup[:, :n], present[:, :n])


@pytest.mark.parametrize("n", [64, 65, 130])
def test_fit_tracker_camera_counts(angles, n):
    run = tws.first_cameras(tws.fit_run(tws.angles_key(angles)), n)
    cams, model, (frames, poses, sup, present) = fit_pair(n)
    with cams, model, fit.FitTracker(cams, model, W, H, params=fit.fit_track_params(**tws.TRACK)) as tr:
        for k in range(tws.FIT_STEPS):
            got = tr.step_poses(frames[k], poses[k], sup[k], present[k], fit.fit_params(**tws.FIT))
            same_records(got, run.records[k], f"records of step {k}")
            same_records(tr.state(), run.state[k], f"state after step {k}")
            assert kinds(got) == tws.fit_kinds(n)[k]


def test_fit_tracker_device_form_65_cameras_between_guard_bands(angles):
    """Step 1 -- the step of every kind -- as a _device step on a side stream with the records between guard bands."""
    import torch
    n = 65
    run = tws.first_cameras(tws.fit_run(tws.angles_key(angles)), n)
    cams, model, (frames, poses, sup, present) = fit_pair(n)
    stream = torch.cuda.Stream()
    with cams, model, fit.FitTracker(cams, model, W, H, params=fit.fit_track_params(**tws.TRACK)) as th, \
            fit.FitTracker(cams, model, W, H, params=fit.fit_track_params(**tws.TRACK)) as td:
        for t in (th, td):
            same_records(t.step_poses(frames[0], poses[0], sup[0], present[0], fit.fit_params(**tws.FIT)), run.records[0], "step 0")
        want = th.step_poses(frames[1], poses[1], sup[1], present[1], fit.fit_params(**tws.FIT))
        d_in = [to_device(a) for a in (frames[1], poses[1], sup[1], present[1])]
        rec, rec_p, rec_o = guarded(n * FIT_REC.itemsize, 8)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            td.step_device(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), rec_p, present_ptr=d_in[3].data_ptr(),
                           fit_params=fit.fit_params(**tws.FIT), stream=stream.cuda_stream)
        stream.synchronize()
        assert untouched(rec, rec_o, n * FIT_REC.itemsize)
        got = rec.cpu().numpy()[rec_o:rec_o + n * FIT_REC.itemsize].view(FIT_REC)
        same_records(got, want, "records of the _device step against the host form")
        same_records(got, run.records[1], "records of the _device step against the restatement")
        same_records(td.state(), th.state(), "state")
        same_records(td.state(), run.state[1], "state against the restatement")
