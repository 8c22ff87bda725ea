"""The subject fit tracker on the GPU against its restatement (tests/subject_track_ref.py): every byte of every
record and of the state after every step -- no tolerance.  Three cameras of 160x120 (one with a matrix that is no pinhole) over
a gallery of three enrolled subjects and one that is not, six steps with a head gone and back, an absent camera and an invalid
detection; want counts of 0, 1 and all cameras; more wanted pairs than the score grid has workgroups, with a staged and a
streamed model; galleries of 1, 63, 64 and 65; nobody enrolled; every bound and unbound start kind in one launch; the set updated
on the stream between two steps; the identification half against dh_fit_identify_subjects_cameras_device; the host calls against
their _device twins on a side stream between guard bands; resets; two runs of one sequence; one step captured in a graph; the
refusals that need a tracker; and the test the feature exists for: a bound camera is fitted with its subject's model."""
import ctypes as C
import functools

import numpy as np
import pytest

import fit_ref as fr
import fit_track_ref as ft
import fit_track_scenes as fts
import ident_ref as ir
import subject_track_ref as stf
import subject_track_scenes as sts
from depthhead_amd import _lib, fit, tracking
from gpu_kit import guarded, same_records, to_device, untouched
from subject_track_gpu import IDENT, TRACK, both, gpu_set, pair

pytestmark = pytest.mark.gpu

W, H, STEPS = 160, 120, 6
REC, STATE, POSE, SUP = _lib.SUBJECT_TRACK_RECORD_DTYPE, _lib.SUBJECT_TRACK_STATE_DTYPE, _lib.POSE_DTYPE, _lib.SUPPORT_DTYPE
UNKNOWN = stf.UNKNOWN
EINVAL = -1


def k_keys():
    from depthhead_amd import synth
    K = synth.default_intrinsic(W, H)
    Ks = np.stack([K, K, K]).astype(np.float32)
    Ks[1, 0, 0] *= 1.3; Ks[1, 1, 1] *= 0.8; Ks[1, 0, 2] += 11.5
    Ks[2, 0, 1] = 3.0; Ks[2, 2, 0] = 1e-4                             # a matrix that is no pinhole
    return tuple(tuple(k.reshape(9).tolist()) for k in Ks)


@functools.lru_cache(maxsize=None)
def main_sequence():
    """Four subjects, 0 .. 2 enrolled.  Camera 0 shows subject 1; camera 1 subject 3, who is not enrolled, gone at steps 3 and 4
    and its detection invalid at step 4; camera 2 (no pinhole) the stranger, absent at steps 2 - 3, its detection invalid at step 0."""
    frames, Ks, _, _, poses = sts.sequence("642", 4, W, H, (1, 3, sts.STRANGER), STEPS, gone=((3, 1), (4, 1)), K_keys=k_keys())
    sup = np.stack([fts.good_support(3) for _ in range(STEPS)])
    sup["mass"][4, 1] = 0
    sup["windows"][0, 2] = 0
    present = np.ones((STEPS, 3), np.uint8)
    present[2:4, 2] = 0
    for a in (sup, present):
        a.setflags(write=False)
    return frames, Ks, poses, sup, present


@pytest.fixture(scope="module")
def angles():
    return fit.angles()


def kinds(rec):
    return (np.asarray(rec["track"]["status"]) & 0xFF).tolist()


def run_both(tr, ref, frames, poses, sup, present=None, steps=None):
    return np.stack([both(tr, ref, frames[k], poses[k], sup[k] if sup.ndim > 1 else sup, None if present is None else present[k], f"step {k}")
                     for k in range(len(frames) if steps is None else steps)])


def test_bound_camera_is_fitted_with_its_subjects_model(angles):
    """Fails without the feature: no such export exists, and a FitTracker with the generic model gives another record."""
    frames, Ks, _, _, poses = sts.sequence("642", 3, 96, 96, (0, 2), 3)
    sup = fts.good_support(2)
    with pair(angles, "642", 3, Ks, 96, 96) as (tr, ref, got, st, cams, model), fit.FitTracker(cams, model, 96, 96, params=fit.fit_track_params(**TRACK)) as plain:
        init = tr.state()
        assert (init["subject"] == UNKNOWN).all() and not np.frombuffer(init["fit"].tobytes(), np.uint8).any() and not init["wait"].any()
        rec = run_both(tr, ref, frames, poses, fts.good_support(2))
        generic = np.stack([plain.step_poses(frames[k], poses[k], sup) for k in range(3)])
    assert rec["subject"].tolist() == [[0, 2]] * 3 and rec["model"].tolist() == [[UNKNOWN, UNKNOWN], [0, 2], [0, 2]]
    assert rec["track"]["instance"]["mesh"].tolist() == [[3, 3], [0, 2], [0, 2]]
    assert rec["track"]["fit"][0].tobytes() == generic["fit"][0].tobytes()                       # step 0 IS the generic tracker's fit
    for k in (1, 2):
        for c in (0, 1):
            assert rec["track"]["fit"][k, c].tobytes() != generic["fit"][k, c].tobytes()
            own = rec["track"]["fit"][k, c]["sum_r2_fixed"] / rec["track"]["fit"][k, c]["points"]
            assert own < generic["fit"][k, c]["sum_r2_fixed"] / generic["fit"][k, c]["points"]
            # and it is the fit of subject c's model, started from the state
            Rf, tf, r = fr.fit(frames[k, c], Ks[c], st.pts[(0, 2)[c]], st.nrm[(0, 2)[c]], rec["track"]["instance"]["R"][k - 1, c].reshape(3, 3),
                               rec["track"]["instance"]["t"][k - 1, c], np.float32(1.0), fr.params(coarse_iterations=0, iterations=6))
            assert (r["points"], r["sum_r2_fixed"]) == (rec["track"]["fit"]["points"][k, c], rec["track"]["fit"]["sum_r2_fixed"][k, c])


def test_main_sequence_three_cameras(angles):
    frames, Ks, poses, sup, present = main_sequence()
    with pair(angles, "642", 4, Ks, W, H, enrolled=[1, 1, 1, 0], sub=dict(retry=1, max_tries=2)) as (tr, ref, *_):
        rec = run_both(tr, ref, frames, poses, sup, present)
    F, Cc, R, N, A = ft.FITTED, ft.CARRIED, ft.REJECTED, ft.NONE, ft.ABSENT
    print([kinds(r) for r in rec], rec["subject"].tolist(), rec["identified"].tolist(), rec["ident"]["status"].tolist())
    assert [kinds(r)[0] for r in rec] == [F, Cc, Cc, Cc, Cc, Cc] and rec["subject"][:, 0].tolist() == [1] * 6
    assert [kinds(r)[1] for r in rec] == [F, Cc, Cc, R, N, F]
    assert [kinds(r)[2] for r in rec][:4] == [N, F, A, A]
    assert 3 not in rec["subject"].ravel().tolist() and (rec["ident"]["best"][rec["identified"] == 1] != 3).all()
    assert rec["identified"][:, 0].tolist() == [1, 0, 0, 0, 0, 0] and rec["identified"][0, 2] == 0 and rec["identified"][1, 2] == 1


def test_motion_flag_and_a_surface_set(angles):
    frames, Ks, poses, sup, present = main_sequence()
    with pair(angles, "642", 4, Ks, W, H, surface=True, flags=ft.MOTION, sub=dict(retry=0, max_tries=0), ident=dict(IDENT, iterations=2, min_ratio=1.02)) as (tr, ref, *_):
        rec = run_both(tr, ref, frames, poses, sup, present)
    assert rec["identified"].any()


def test_want_counts_of_all_none_and_one(angles):
    frames, Ks, _, _, poses = sts.sequence("642", 3, 96, 96, (0, 1, 2), 3)
    sup = fts.good_support(3)
    with pair(angles, "642", 3, Ks, 96, 96) as (tr, ref, *_):
        r0 = both(tr, ref, frames[0], poses[0], sup)
        r1 = both(tr, ref, frames[1], poses[1], sup)
        tr.reset(1); ref.reset(1)
        r2 = both(tr, ref, frames[2], poses[2], sup)
    assert [int(r["identified"].sum()) for r in (r0, r1, r2)] == [3, 0, 1] and r2["identified"].tolist() == [0, 1, 0]
    assert r2["subject"].tolist() == [0, 1, 2] and r2["model"].tolist() == [0, UNKNOWN, 2]


@pytest.mark.parametrize("name,points", [("257", 257), ("lathe31x33", 1025)])
def test_more_wanted_pairs_than_the_score_grid_has_workgroups(angles, name, points):
    """Every camera wants identification against 64 candidates, and the cameras are one more than fill the grid: some workgroup
    makes a second trip, staged (257 points) or streamed (1025 points: above the LDS budget).  Where the grid is a multiple of 64
    -- 512 on an MI355X -- that second trip has the SAME subject as the first and only the instance changes, so this shows a second
    trip, not a second model: a model staged on the first trip only would pass.  test_gpu_score_trips.py has the trips whose
    subject changes.  One set holds models of one size, so the two kinds alternate over the two cases, not within a step."""
    import torch
    S = 64
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    n = grid // S + 1
    frames, Ks, _, _, poses = sts.sequence(name, S, 96, 96, tuple((7 * c) % S for c in range(n)), 1)
    assert len(sts.mesh(name)[0]) == points
    track = dict(rms_max=4096.0, keep_points=1, max_jump=4096.0)
    with pair(angles, name, S, Ks, 96, 96, track=track, ident=dict(min_points=16, max_rms=np.inf)) as (tr, ref, *_):
        assert tr.info() == (n, S, grid) and n * S > grid
        rec = both(tr, ref, frames[0], poses[0], fts.good_support(n))
    assert (rec["identified"] == 1).all() and (rec["ident"]["eligible"] == S).all(), (kinds(rec), rec["ident"]["eligible"])


@pytest.mark.parametrize("n_subjects", [1, 63, 64, 65])
def test_gallery_sizes_about_the_bind_waves_stride(angles, n_subjects):
    who = (n_subjects // 2, n_subjects - 1)
    frames, Ks, _, _, poses = sts.sequence("642", n_subjects, 96, 96, who, 2)
    with pair(angles, "642", n_subjects, Ks, 96, 96, ident=dict(min_points=16, max_rms=np.inf)) as (tr, ref, *_):
        assert tr.info()[:2] == (2, n_subjects)
        rec = run_both(tr, ref, frames, poses, fts.good_support(2))
    assert (rec["ident"]["eligible"][0] == n_subjects).all() and (rec["ident"]["status"][0] == ir.OK).all()
    assert ((rec["ident"]["second"][0] == UNKNOWN) == (n_subjects == 1)).all() and (rec["model"][1] == rec["subject"][0]).all()


def test_nobody_enrolled_and_the_mask_replaced(angles):
    frames, Ks, _, _, poses = sts.sequence("642", 3, 96, 96, (0, 2), 4)
    sup = fts.good_support(2)
    with pair(angles, "642", 3, Ks, 96, 96, enrolled=[0, 0, 0], sub=dict(retry=0, max_tries=0)) as (tr, ref, *_):
        r0 = both(tr, ref, frames[0], poses[0], sup)
        assert (r0["ident"]["status"] == ir.NO_CANDIDATE).all() and (r0["subject"] == UNKNOWN).all() and r0["tries"].tolist() == [1, 1]
        tr.set_enrolled([0, 0, 1]); ref.set_enrolled([0, 0, 1])
        r1 = both(tr, ref, frames[1], poses[1], sup)
        assert r1["subject"].tolist() == [UNKNOWN, 2] and r1["ident"]["eligible"].tolist() == [1, 1]
        tr.set_enrolled(None); ref.set_enrolled(None)
        r2 = both(tr, ref, frames[2], poses[2], sup)
        assert r2["subject"].tolist() == [0, 2] and r2["identified"].tolist() == [1, 0]


def test_every_bound_and_unbound_start_kind_in_one_launch(angles):
    """Camera 0: carried and bound; camera 1: carried and unbound (a stranger); camera 2: detected and unbound; camera 3: detected
    and bound by the caller; camera 4 a bound camera rejected."""
    frames, Ks, _, _, poses = sts.sequence("642", 3, 96, 96, (0, sts.STRANGER, 1, 2, 2), 2, gone=((1, 4),))
    sup = fts.good_support(5)
    with pair(angles, "642", 3, Ks, 96, 96, sub=dict(retry=0, max_tries=0)) as (tr, ref, *_):
        both(tr, ref, frames[0], poses[0], sup)
        for c in (2, 3):
            tr.reset(c); ref.reset(c)
        tr.bind(3, 2); ref.bind(3, 2)
        same_records(tr.state(), ref.state, "state after the reset and the bind")
        rec = both(tr, ref, frames[1], poses[1], sup)
    assert kinds(rec) == [ft.CARRIED, ft.CARRIED, ft.FITTED, ft.FITTED, ft.REJECTED]
    assert rec["model"].tolist() == [0, UNKNOWN, UNKNOWN, 2, 2] and rec["identified"].tolist() == [0, 1, 1, 0, 0]
    assert rec["subject"].tolist() == [0, UNKNOWN, 1, 2, UNKNOWN]


def test_the_set_updated_on_the_stream_between_two_steps(angles):
    """dh_fit_subjects_update_device between two _device steps on one stream: the second step's fit is the restatement's at the
    updated model (the tracker's table names the set's buffers, which the update rewrites in place)."""
    import torch
    frames, Ks, _, _, poses = sts.sequence("642", 3, 96, 96, (0, 2), 2)
    sup = fts.good_support(2)
    shape = np.zeros(3, _lib.SHAPE_RECORD_DTYPE)
    shape["delta"][:, 0] = [0.08, 0.0, -0.11]
    shape["points"], shape["instances"] = 100, 1
    with pair(angles, "642", 3, Ks, 96, 96) as (tr, ref, got, st, *_):
        stream = torch.cuda.Stream()
        d_rec = [torch.zeros(2 * REC.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_in = [(to_device(frames[k]), to_device(poses[k]), to_device(sup)) for k in range(2)]
        d_shape = to_device(shape)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            tr.step_device(d_in[0][0].data_ptr(), d_in[0][1].data_ptr(), d_in[0][2].data_ptr(), d_rec[0].data_ptr(), stream=stream.cuda_stream)
            got.update(d_shape, device=True, stream=stream.cuda_stream)
            tr.step_device(d_in[1][0].data_ptr(), d_in[1][1].data_ptr(), d_in[1][2].data_ptr(), d_rec[1].data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        before = st.pts[0].copy()
        want0 = ref.step(frames[0], poses[0], sup)
        st.update(shape)
        assert st.pts[0].tobytes() != before.tobytes() and got.read(0)[0].tobytes() == st.pts[0].tobytes()
        want1 = ref.step(frames[1], poses[1], sup)
        same_records(d_rec[0].cpu().numpy().view(REC), want0, "step 0")
        same_records(d_rec[1].cpu().numpy().view(REC), want1, "step 1, after the update")
        same_records(tr.state(), ref.state, "state")
    assert want1["model"].tolist() == [0, 2]


def test_the_identification_half_equals_the_existing_call(angles):
    """The list kernel held to dh_fit_identify_subjects_cameras_device: the step's fitted instances with the fit records of the
    cameras that did not want identification marked not-OK give the same dh_ident_record for every camera that did."""
    import torch
    frames, Ks, poses, sup, present = main_sequence()
    enrolled = np.array([1, 1, 1, 0], np.uint8)
    with pair(angles, "642", 4, Ks, W, H, enrolled=enrolled, sub=dict(retry=0, max_tries=0)) as (tr, ref, got, st, cams, model), fit.Fitter() as ftr:
        seen = 0
        for k in range(3):
            rec = both(tr, ref, frames[k], poses[k], sup[k], present[k], f"step {k}")
            frec = rec["track"]["fit"].copy()
            frec["status"][rec["identified"] == 0] = fr.FEW_POINTS
            d_frames = torch.from_numpy(frames[k].view(np.int16).copy()).cuda()
            out = ftr.identify_subjects(d_frames, got, to_device(rec["track"]["instance"]), cams, enrolled=to_device(enrolled), fit_records=to_device(frec),
                                        params=fit.ident_params(**IDENT), device_out=True)
            torch.cuda.synchronize()
            subjects, irec = out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy().view(_lib.IDENT_RECORD_DTYPE)
            for c in range(3):
                if rec["identified"][c]:
                    assert irec[c].tobytes() == rec["ident"][c].tobytes(), (k, c, irec[c], rec["ident"][c])
                    assert subjects[c] == rec["subject"][c]
                    seen += 1
                else:
                    assert irec[c]["status"] == ir.SKIPPED == rec["ident"][c]["status"]
        assert seen >= 3


@functools.lru_cache(maxsize=None)
def forest():
    from depthhead_amd import synth
    return synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)


def test_host_calls_against_device_twins_between_guard_bands(angles):
    """The core step and the whole step, host call against _device twin on a side stream; the twin's outputs lie between 4 KB
    guard bands at skewed pointers (8 bytes off for the records, the poses and the support) and nothing outside them changes."""
    import torch
    from depthhead_amd import prediction, synth
    frames, Ks, poses, sup, present = main_sequence()
    stream = torch.cuda.Stream()
    with prediction.HoughPrediction(forest(), synth.ModelParams(stepwidth=4)) as hp, \
            pair(angles, "642", 4, Ks, W, H, enrolled=[1, 1, 1, 0], trackers=4) as ((th, td, wh, wd), ref, *_):
        for k in range(4):
            want = th.step_poses(frames[k], poses[k], sup[k], present[k])
            same_records(want, ref.step(frames[k], poses[k], sup[k], present[k]), f"host records of step {k}")
            w_poses, w_sup, w_rec = wh.step(hp, frames[k], present[k])
            d_frames, d_poses, d_sup, d_pr = to_device(frames[k]), to_device(poses[k]), to_device(sup[k]), to_device(present[k])
            rec, rec_p, rec_o = guarded(3 * REC.itemsize, 8)
            rec2, rec2_p, rec2_o = guarded(3 * REC.itemsize, 24)
            po, po_p, po_o = guarded(3 * POSE.itemsize, 8)
            so, so_p, so_o = guarded(3 * SUP.itemsize, 8)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                td.step_device(d_frames.data_ptr(), d_poses.data_ptr(), d_sup.data_ptr(), rec_p, present_ptr=d_pr.data_ptr(), stream=stream.cuda_stream)
                wd.step_device(d_frames.data_ptr(), po_p, so_p, rec2_p, hp=hp, present_ptr=d_pr.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            for buf, off, dt, ref_bytes, what in ((rec, rec_o, REC, want, "core records"), (rec2, rec2_o, REC, w_rec, "whole-step records"),
                                                  (po, po_o, POSE, w_poses, "poses"), (so, so_o, SUP, w_sup, "support")):
                nb = 3 * dt.itemsize
                assert untouched(buf, off, nb), what
                same_records(buf.cpu().numpy()[off:off + nb].view(dt), ref_bytes, f"{what} of step {k}")
            same_records(td.state(), th.state(), "core state"); same_records(wd.state(), wh.state(), "whole-step state")


def test_reset_and_two_runs_of_one_sequence(angles):
    frames, Ks, poses, sup, present = main_sequence()
    with pair(angles, "642", 4, Ks, W, H, enrolled=[1, 1, 1, 0]) as (tr, ref, *_):
        first = run_both(tr, ref, frames, poses, sup, present)
        state = tr.state()
        tr.reset(0); ref.reset(0)
        same_records(tr.state(), ref.state, "state after the reset of camera 0")
        assert tr.state()[0].tobytes() == stf.initial(1)[0].tobytes() and tr.state()[1].tobytes() == state[1].tobytes()
        run_both(tr, ref, frames, poses, sup, present, steps=2)
        tr.reset(); ref.reset()
        assert tr.state().tobytes() == stf.initial(3).tobytes()
        second = run_both(tr, ref, frames, poses, sup, present)
        assert first.tobytes() == second.tobytes() and tr.state().tobytes() == state.tobytes()


def test_one_step_captured_in_a_graph(angles):
    """The core step's five launches, a linear chain, captured with torch.cuda.graph; each replay is one step and equals the eager step."""
    import torch
    frames, Ks, _, _, poses = sts.sequence("642", 3, 96, 96, (0, sts.STRANGER, 2), 3)
    sup = fts.good_support(3)
    with pair(angles, "642", 3, Ks, 96, 96, sub=dict(retry=1, max_tries=0), trackers=2) as ((eager, tr), ref, *_):
        d_frames, d_poses, d_sup = to_device(frames[0]), to_device(poses[0]), to_device(sup)
        d_rec = torch.zeros(3 * REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tr.step_device(d_frames.data_ptr(), d_poses.data_ptr(), d_sup.data_ptr(), d_rec.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        tr.reset()                                                     # whatever the capture itself ran or did not run
        torch.cuda.synchronize()
        for k in range(3):
            d_frames.copy_(to_device(frames[k])); d_poses.copy_(to_device(poses[k]))
            g.replay()
            torch.cuda.synchronize()
            want = eager.step_poses(frames[k], poses[k], sup)
            same_records(want, ref.step(frames[k], poses[k], sup), f"eager step {k}")
            same_records(d_rec.cpu().numpy().view(REC), want, f"replay {k}")
            same_records(tr.state(), eager.state(), f"state after replay {k}")


def test_refusals_that_need_a_tracker(angles):
    frames, Ks, _, _, poses = sts.sequence("642", 3, 96, 96, (0, 2), 2)
    sup = fts.good_support(2)
    lib, vp = _lib.load(), _lib.vp
    with pair(angles, "642", 3, Ks, 96, 96) as (tr, ref, got, st, cams, model):
        tr.step_poses(frames[0], poses[0], sup)
        state = tr.state()
        rec = np.full(2 * REC.itemsize, 0xCD, np.uint8)
        f, p, s = np.ascontiguousarray(frames[1]), np.ascontiguousarray(poses[1]), np.ascontiguousarray(sup)

        def refused(what, fr_=f, w=96, h=96, po=p, su=s, prm=None, out=rec):
            for name, extra in (("dh_subject_fit_tracker_step_poses", ()), ("dh_subject_fit_tracker_step_poses_device", (None,))):
                rc = getattr(lib, name)(tr._h, vp(fr_), w, h, None, vp(po), vp(su), prm, vp(out), *extra)
                msg = lib.dh_last_error().decode()
                assert rc == EINVAL and what in msg and name in msg, (name, rc, msg)
            assert (rec == 0xCD).all()

        refused("NULL frames", fr_=None)
        refused("NULL poses or support", po=None)
        refused("NULL poses or support", su=None)
        refused("NULL records", out=None)
        for w, h in ((0, 96), (96, 0), (96, _lib.RENDER_MAX_SIZE + 1)):
            refused("frame size", w=w, h=h)
        for kw, what in ((dict(coarse_iterations=33, iterations=32), "above 64"), (dict(gate=(0.0, 25.0)), "gate[0]"), (dict(min_points=5), "min_points 5 below 6")):
            refused(what, prm=C.byref(fit.fit_params(**kw)))
        for cam in (-2, 2):
            with pytest.raises(_lib.DepthheadError) as ei:
                tr.reset(cam)
            assert ei.value.code == EINVAL and "camera" in str(ei.value)
        for cam, subject, what in ((-1, 0, "camera -1"), (2, 0, "camera 2"), (0, 3, "subject 3"), (0, 0xFFFFFFFE, "subject")):
            with pytest.raises(_lib.DepthheadError) as ei:
                tr.bind(cam, subject)
            assert ei.value.code == EINVAL and what in str(ei.value)
        assert lib.dh_subject_fit_tracker_state(tr._h, None) == EINVAL and "NULL" in lib.dh_last_error().decode()
        assert lib.dh_subject_fit_tracker_info(tr._h, None, None, None) == 0
        assert tr.state().tobytes() == state.tobytes()                 # nothing was launched
        # ---- creation's refusals past the handles, in the header's order: each with the later faults present too
        h = C.c_void_p(1234)
        wrong = fit.Model(*sts.generic("162"))
        big = float(np.float32(4096.5 / got.info()[4]))

        def create(what, scale=1.0, ident=None, sub=None, m=model, enrolled=None):
            rc = lib.dh_subject_fit_tracker_create(cams._h, got._h, m._h, C.c_float(scale), C.c_uint32(0), None, _lib.ref(ident), _lib.ref(sub),
                                                   vp(enrolled), C.byref(h))
            msg = lib.dh_last_error().decode()
            assert rc == EINVAL and what in msg and "dh_subject_fit_tracker_create" in msg and h.value is None, (what, rc, msg)

        bad_sub = _lib.SubjectTrackParams()
        bad_sub.reserved[0] = 1
        create("iterations = 65 above 64", scale=big, ident=fit.ident_params(iterations=65), sub=bad_sub, m=wrong)
        create("min_ratio", scale=big, ident=fit.ident_params(min_ratio=0.5), sub=bad_sub, m=wrong)
        create("reserved word of the dh_subject_track_params", scale=big, sub=bad_sub, m=wrong)
        create("the generic model has 162 points, a model of the set 642", scale=big, m=wrong)
        create("a model of the set may span", scale=big)
        create("a model of the set may span", scale=-big)
        wrong.close()
        far = np.asarray(sts.generic("642")[0]) * np.float32(3.0)         # a generic model larger than the set's bound
        with fit.Model(far, sts.generic("642")[1]) as wide:
            scale = float(np.float32(4096.5 / wide.info()[1]))
            assert scale * got.info()[4] <= 4096.0
            create("the model spans", scale=scale, m=wide)
    # one pair above DH_IDENT_MAX_PAIRS: 16 385 cameras times 256 subjects (refused before anything is allocated)
    with gpu_set("4", 256) as (big_set, _), tracking.Cameras(np.stack([Ks[0]] * 16385)) as many, fit.Model(*sts.generic("4")) as tetra:
        h = C.c_void_p(1234)
        rc = lib.dh_subject_fit_tracker_create(many._h, big_set._h, tetra._h, C.c_float(1.0), C.c_uint32(0), None, None, None, None, C.byref(h))
        assert rc == EINVAL and "16385 cameras times 256 subjects exceed 4194304 pairs" in lib.dh_last_error().decode() and h.value is None
        with tracking.Cameras(np.stack([Ks[0]] * 2)) as two, fit.SubjectFitTracker(two, big_set, tetra, 96, 96) as tr:
            assert tr.info()[:2] == (2, 256)
