"""The rig subject fit tracker on the GPU against its restatement (tests/rig_subject_track_ref.py): every byte of
every record and of the state after every step -- no tolerance.  Splatted rigs of small frames (96x96, 64x48) over galleries of 162,
257 and 1 025 vertices: two rigs of 3 and 2 cameras with three enrolled subjects and one that is not, six steps with a person gone
and back, an absent camera, a wholly absent rig, two people in one rig, an unbound person and a person that names no head; the same
on a surface set with the motion flag; want counts of several, 0 and 1 with wanting slots in the first lane, the last lane and
across a wave boundary of the update kernel; more wanted pairs than the score grid has workgroups, staged and streamed; galleries of
1, 63, 64 and 65; nobody enrolled; the set updated on the stream between two steps; the identification half against
dh_fit_identify_subjects_views_device; the host calls against their _device twins on a side stream between guard bands; resets; two
runs of one sequence; one step captured in a graph; one whole step behind a real RigTracker; a one-camera rig through the identity
against SubjectFitTracker; the refusals that need a tracker; and the test the feature exists for: a bound person is fitted with its
subject's model."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import fit_ref as fr
import fit_track_ref as ft
import fit_track_scenes as fts
import ident_ref as ir
import ident_views_ref as ivr
import rig_fit_track_ref as rf
import rig_subject_track_ref as rs
import rig_subject_track_scenes as sc
import subject_track_scenes as sts
import view_fit_ref as vr
from depthhead_amd import _lib, fit, tracking
from gpu_kit import guarded, same_records, to_device, untouched
from subject_track_gpu import gpu_set

pytestmark = pytest.mark.gpu

REC, STATE = _lib.RIG_SUBJECT_RECORD_DTYPE, _lib.RIG_SUBJECT_STATE_DTYPE
SLOTS = _lib.RIG_MAX_TRACKS
UNKNOWN = rs.UNKNOWN
EINVAL = -1
F, Cd, R, N, A = rf.FITTED, rf.CARRIED, rf.REJECTED, rf.NONE, rf.ABSENT
# The splatted small frames are coarse (tests/test_rig_subject_track_ref.py): the tracker believes a fit up to 8 mm, and where a test
# is about who binds the identification's limit lies between a known head's best mean square and the stranger's.
TRACK = dict(rms_max=8.0)
IDENT = dict(min_points=16, max_rms=3.8)
ANY = dict(min_points=16, max_rms=np.inf)         # whoever is best binds: the test is about the bytes


@pytest.fixture(scope="module")
def angles():
    return fit.angles()


def rig_extrinsics(V, u):
    """The camera-to-world R, t a rig table takes, from the view table's V, u (only rig_begin matters to the fit tracker)."""
    Rm = np.transpose(np.asarray(V, np.float64), (0, 2, 1))
    return Rm.astype(np.float32), (-np.einsum("nij,nj->ni", Rm, np.asarray(u, np.float64))).astype(np.float32)


@contextlib.contextmanager
def pair(angles, name, n_subjects, s, enrolled=None, sub=None, track=None, ident=None, surface=False, flags=0, trackers=1):
    """(trackers on the GPU, the restated tracker, the GPU set, the restated set, cameras, rig, views, model) over scene s."""
    track, ident = dict(TRACK if track is None else track), dict(IDENT if ident is None else ident)
    with contextlib.ExitStack() as stack:
        got, st = stack.enter_context(gpu_set(name, n_subjects, surface))
        cams = stack.enter_context(tracking.Cameras(s.Ks))
        rig = stack.enter_context(tracking.Rig(cams, *rig_extrinsics(s.V, s.u), s.rig_begin))
        views = stack.enter_context(fit.Views(cams, s.V, s.u))
        model = stack.enter_context(fit.Model(*sts.generic(name)))
        trs = [stack.enter_context(fit.RigSubjectFitTracker(rig, views, got, model, s.w, s.h, motion=bool(flags),
                                                            params=fit.rig_fit_track_params(**track), ident_params=fit.ident_views_params(**ident),
                                                            subject_params=None if sub is None else fit.subject_track_params(**sub),
                                                            enrolled=enrolled)) for _ in range(trackers)]
        ref = rs.Tracker(s.Ks, s.V, s.u, s.rig_begin, st, sts.generic(name), angles, flags=flags, prm=rf.params(**track),
                         ident_prm=ivr.params(**ident), sub_prm=None if sub is None else rs.params(**sub), enrolled=enrolled)
        yield trs if trackers > 1 else trs[0], ref, got, st, cams, rig, views, model


def both(tr, ref, s, k, items, present=None, what=None, fit_kw=None):
    """One step on the GPU (host call) and in the restatement; records and state compared."""
    inputs = s.inputs(items)
    got = tr.step_persons(s.frames[k], *inputs, present=present, fit_params=None if fit_kw is None else fit.fit_params(**fit_kw))
    want = ref.step(s.frames[k], *inputs, present=present, fit_prm=None if fit_kw is None else fr.params(**fit_kw))
    assert got.dtype == REC and got.shape == (s.n_rigs, SLOTS)
    same_records(got, want, f"records of {what or f'step {k}'}")
    same_records(tr.state(), ref.state, f"state after {what or f'step {k}'}")
    return got


def kinds(rec):
    return (np.asarray(rec["track"]["status"]) & 0xFF).tolist()


def test_bound_person_is_fitted_with_its_subjects_model(angles):
    """Fails without the feature: no such export exists, and a RigFitTracker with the generic model gives another record."""
    s = sc.scene("162", 3, 96, 96, ((3, (0, 2)),), 3)
    items = lambda k: [s.item(k, 0, 0, 7, best=k % 3), s.item(k, 0, 1, 9, best=1)]
    with pair(angles, "162", 3, s, ident=ANY) as (tr, ref, got, st, cams, rig, views, model), \
            fit.RigFitTracker(rig, views, model, 96, 96, params=fit.rig_fit_track_params(**TRACK)) as plain:
        init = tr.state()
        assert (init["subject"] == UNKNOWN).all() and not np.frombuffer(init["fit"].tobytes(), np.uint8).any() and not init["wait"].any()
        rec = np.stack([both(tr, ref, s, k, items(k))[0, :2] for k in range(3)])
        generic = np.stack([plain.step_persons(s.frames[k], *s.inputs(items(k)))[0, :2] for k in range(3)])
    bound = rec["subject"][0].tolist()
    assert all(b < 3 for b in bound) and rec["subject"].tolist() == [bound] * 3 and rec["identified"].tolist() == [[1, 1], [0, 0], [0, 0]]
    assert rec["model"].tolist() == [[UNKNOWN, UNKNOWN], bound, bound] and rec["track"]["instance"]["model"].tolist() == [[3, 3], bound, bound]
    assert rec["track"]["fit"][0].tobytes() == generic["fit"][0].tobytes()                       # step 0 IS the generic tracker's fit
    for k in (1, 2):
        for j in (0, 1):
            if bound[j] != 1:                                                                    # (subject 1 of three IS the generic head)
                assert rec["track"]["fit"][k, j].tobytes() != generic["fit"][k, j].tobytes()
            # it is the multi-view fit of the bound subject's model, started from the state
            prev = rec["track"]["instance"][k - 1, j]
            Rf, tf, r = vr.fit(s.frames[k], s.Ks, s.V, s.u, 0, int(rec["track"]["instance"]["views"][k, j]), st.pts[bound[j]], st.nrm[bound[j]],
                               prev["R"].reshape(3, 3), prev["t"], np.float32(1.0), fr.params(coarse_iterations=0, iterations=6))
            assert (r["points"], r["sum_r2_fixed"]) == (rec["track"]["fit"]["points"][k, j], rec["track"]["fit"]["sum_r2_fixed"][k, j])
    assert any(b != 1 for b in bound)


@functools.lru_cache(maxsize=None)
def main_scene():
    """Rig 0 (3 cameras): person 0 is subject 1 under id 7, person 1 is subject 3 (not enrolled) under id 8, gone at steps 3 and 4.
    Rig 1 (2 cameras): the stranger under id 0 (unbound), and from step 2 on person 1, subject 0 under id 5."""
    return sc.scene("162", 4, 96, 96, ((3, (1, 3)), (2, (sc.STRANGER, 0))), 6, gone=((3, 0, 1), (4, 0, 1)))


def main_steps(s):
    """Per step (items, present): an absent camera at step 1, rig 1 wholly absent at step 2, person (0, 1) gone at steps 3 and 4 and
    back at 5, a person that names no head at step 4."""
    out = []
    for k in range(6):
        items = [s.item(k, 0, 0, 7, best=k % 3)]
        if k not in (3, 4):
            items.append(s.item(k, 0, 1, 8, best=1))
        items.append(s.item(k, 1, 0, 0, best=0))
        if k >= 2:
            items.append(s.item(k, 1, 1, 5, best=1, head=1 if k != 4 else sc.rsc.MAX_HEADS))
        present = {1: [1, 0, 1, 1, 1], 2: [1, 1, 1, 0, 0]}.get(k)
        out.append((items, present))
    return out


def run_main(tr, ref, s, steps=6):
    recs = []
    for k, (items, present) in enumerate(main_steps(s)[:steps]):
        if k == 4:                                         # best_head = max_heads names no head: rig_inputs would not place it
            g, p, hd = items[-1]
            p = p.copy()
            keep = items[:-1]
            inputs = list(s.inputs(keep))
            inputs[3][g, inputs[2][g]] = p
            inputs[2][g] += 1
            got = tr.step_persons(s.frames[k], *inputs, present=present)
            want = ref.step(s.frames[k], *inputs, present=present)
            same_records(got, want, "records of step 4"); same_records(tr.state(), ref.state, "state after step 4")
            recs.append(got)
        else:
            recs.append(both(tr, ref, s, k, items, present))
    return np.stack(recs)


def test_main_sequence_two_rigs(angles):
    s = main_scene()
    with pair(angles, "162", 4, s, enrolled=[1, 1, 1, 0], sub=dict(retry=1, max_tries=2), ident=ANY) as (tr, ref, *_):
        rec = run_main(tr, ref, s)
    print([kinds(r[:, :2]) for r in rec], rec["subject"][:, :, :2].tolist(), rec["identified"][:, :, :2].tolist())
    assert [kinds(r[0])[0] for r in rec] == [F, Cd, Cd, Cd, Cd, Cd]
    assert [kinds(r[0])[1] for r in rec][:4] == [F, Cd, Cd, R] and (rec[2, 1]["track"]["status"] == A).all()
    assert 3 not in rec["subject"].ravel().tolist() and (rec["ident"]["best"][rec["identified"] == 1] != 3).all()
    unbound = rec["track"]["id"][:, 1] == 0
    assert not rec["identified"][:, 1][unbound & (rec["track"]["status"][:, 1] != 0)].any()
    assert rec["identified"][0, 0, :2].tolist() == [1, 1] and rec["identified"][1].sum() == 0


def test_motion_flag_and_a_surface_set(angles):
    s = main_scene()
    with pair(angles, "162", 4, s, surface=True, flags=rf.MOTION, sub=dict(retry=0, max_tries=0),
              ident=dict(min_points=16, max_rms=np.inf, iterations=2, min_ratio=1.02)) as (tr, ref, *_):
        rec = run_main(tr, ref, s)
    assert rec["identified"].any()


def test_want_counts_of_several_none_and_one_at_the_edges_of_the_update_wave(angles):
    """Six one-camera rigs of 64x48: the update kernel's first wave holds rigs 0 - 3.  Rig 0's one person founds slot 0 (the first
    lane); rig 3 reports sixteen ids on one head, so its slot 15 is the wave's last lane, and rig 4's slot 0 opens the second wave:
    the list is appended across the boundary.  Then nobody wants, then one slot alone."""
    s = sc.scene("162", 2, 64, 48, ((1, (0,)), (1, (1,)), (1, (1,)), (1, (1,)), (1, (0,)), (1, (1,))), 3)

    def items(k):
        out = [s.item(k, 0, 0, 3), s.item(k, 4, 0, 4)]
        return out + [s.item(k, 3, 0, 100 + i) for i in range(16)]
    fit_kw = dict(coarse_iterations=1, iterations=3)
    track = dict(rms_max=4096.0, keep_points=1, max_jump=4096.0)
    with pair(angles, "162", 2, s, ident=ANY, track=track) as (tr, ref, *_):
        r0 = both(tr, ref, s, 0, items(0), fit_kw=fit_kw)
        r1 = both(tr, ref, s, 1, items(1), fit_kw=fit_kw)
        tr.reset(4); ref.reset(4)
        r2 = both(tr, ref, s, 2, items(2), fit_kw=fit_kw)
    assert r0["identified"][0].tolist() == [1] + [0] * 15 and r0["identified"][3].all() and r0["identified"][4, 0] == 1
    assert int(r0["identified"].sum()) == 18 and int(r1["identified"].sum()) == 0 and int(r2["identified"].sum()) == 1
    assert r2["identified"][4, 0] == 1 and (r2["model"][3] == r0["subject"][3]).all()


@pytest.mark.parametrize("name,points,cams,iterations", [("257", 257, 1, 4), ("lathe31x33", 1025, 2, 1)])
def test_more_wanted_pairs_than_the_score_grid_has_workgroups(angles, name, points, cams, iterations):
    """Every slot in use wants identification against 64 candidates, and the slots are one more than fill the grid: some workgroup
    makes a second trip, staged (257 points) or streamed (1025 points: above the LDS budget; 2 views, 1 iteration).  Where the grid
    is a multiple of 64 -- 512 on an MI355X -- that second trip has the SAME subject as the first and only the instance changes, so
    this shows a second trip, not a second model: a model staged on the first trip only would pass.  test_gpu_score_trips.py has
    the trips whose subject changes."""
    import torch
    S = 64
    units = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    n = units // S + 1
    s = sc.scene(name, S, 64, 48, tuple((cams, ((11 * g) % S,)) for g in range(n)), 1)
    assert len(sts.mesh(name)[0]) == points
    track = dict(rms_max=4096.0, keep_points=1, max_jump=4096.0)
    with pair(angles, name, S, s, track=track, ident=dict(ANY, iterations=iterations)) as (tr, ref, *_):
        grid = tr.info()[2]
        assert tr.info()[:2] == (n, S) and grid == min(n * SLOTS * S, units) and n * S > grid
        rec = both(tr, ref, s, 0, [s.item(0, g, 0, 20 + g) for g in range(n)], fit_kw=dict(coarse_iterations=1, iterations=2))
    assert (rec["identified"][:, 0] == 1).all() and (rec["ident"]["eligible"][:, 0] == S).all(), (kinds(rec[:, 0]), rec["ident"]["eligible"][:, 0])


@pytest.mark.parametrize("n_subjects", [1, 63, 64, 65])
def test_gallery_sizes_about_the_bind_waves_stride(angles, n_subjects):
    s = sc.scene("162", n_subjects, 64, 48, ((2, (n_subjects // 2, n_subjects - 1)),), 2)
    with pair(angles, "162", n_subjects, s, ident=ANY) as (tr, ref, *_):
        assert tr.info()[:2] == (1, n_subjects)
        rec = np.stack([both(tr, ref, s, k, [s.item(k, 0, 0, 7), s.item(k, 0, 1, 8)])[0, :2] for k in range(2)])
    assert (rec["ident"]["eligible"][0] == n_subjects).all() and (rec["ident"]["status"][0] == ir.OK).all()
    assert ((rec["ident"]["second"][0] == UNKNOWN) == (n_subjects == 1)).all() and (rec["model"][1] == rec["subject"][0]).all()


def test_nobody_enrolled_and_the_mask_replaced(angles):
    s = sc.scene("162", 3, 96, 96, ((3, (0, 2)),), 3)
    items = lambda k: [s.item(k, 0, 0, 7), s.item(k, 0, 1, 8)]
    with pair(angles, "162", 3, s, enrolled=[0, 0, 0], sub=dict(retry=0, max_tries=0), ident=ANY) as (tr, ref, *_):
        r0 = both(tr, ref, s, 0, items(0))[0, :2]
        assert (r0["ident"]["status"] == ir.NO_CANDIDATE).all() and (r0["subject"] == UNKNOWN).all() and r0["tries"].tolist() == [1, 1]
        tr.set_enrolled([0, 0, 1]); ref.set_enrolled([0, 0, 1])
        r1 = both(tr, ref, s, 1, items(1))[0, :2]
        assert r1["subject"].tolist() == [2, 2] and r1["ident"]["eligible"].tolist() == [1, 1]
        tr.set_enrolled(None); ref.set_enrolled(None)
        tr.bind(0, 7, None); ref.bind(0, 7, None)
        tr.bind(0, 99, 1); ref.bind(0, 99, 1)                          # an id nobody holds
        same_records(tr.state(), ref.state, "state after the binds")
        r2 = both(tr, ref, s, 2, items(2))[0, :2]
        assert r2["identified"].tolist() == [1, 0] and r2["ident"]["eligible"][0] == 3 and r2["model"].tolist() == [UNKNOWN, 2]


def device_inputs(s, k, items, present=None):
    n_heads, heads, n_persons, persons = s.inputs(items)
    d = [to_device(a) for a in (s.frames[k], n_heads, heads, n_persons, persons)]
    return d, heads.shape[1], None if present is None else to_device(np.asarray(present, np.uint8))


def step_dev(tr, d, mh, rec_ptr, d_pr=None, stream=0):
    tr.step_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), rec_ptr, max_heads=mh,
                   present_ptr=0 if d_pr is None else d_pr.data_ptr(), stream=stream)


def test_the_set_updated_on_the_stream_between_two_steps(angles):
    """dh_fit_subjects_update_device between two _device steps on one stream: the second step's fit is the restatement's at the
    updated model (the tracker's table names the set's buffers, which the update rewrites in place)."""
    import torch
    s = sc.scene("162", 3, 96, 96, ((3, (0, 2)),), 2)
    items = lambda k: [s.item(k, 0, 0, 7), s.item(k, 0, 1, 8)]
    shape = np.zeros(3, _lib.SHAPE_RECORD_DTYPE)
    shape["delta"][:, 0] = [0.08, 0.0, -0.11]
    shape["points"], shape["instances"] = 100, 1
    with pair(angles, "162", 3, s, ident=ANY) as (tr, ref, got, st, *_):
        stream = torch.cuda.Stream()
        d_rec = [torch.zeros(SLOTS * REC.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_in = [device_inputs(s, k, items(k)) for k in range(2)]
        d_shape = to_device(shape)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            step_dev(tr, d_in[0][0], d_in[0][1], d_rec[0].data_ptr(), stream=stream.cuda_stream)
            got.update(d_shape, device=True, stream=stream.cuda_stream)
            step_dev(tr, d_in[1][0], d_in[1][1], d_rec[1].data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        before = st.pts[0].copy()
        want0 = ref.step(s.frames[0], *s.inputs(items(0)))
        st.update(shape)
        assert st.pts[0].tobytes() != before.tobytes() and got.read(0)[0].tobytes() == st.pts[0].tobytes()
        want1 = ref.step(s.frames[1], *s.inputs(items(1)))
        same_records(d_rec[0].cpu().numpy().view(REC), want0, "step 0")
        same_records(d_rec[1].cpu().numpy().view(REC), want1, "step 1, after the update")
        same_records(tr.state(), ref.state, "state")
    assert (want1["model"][0, :2] < 3).all()


def test_the_identification_half_equals_the_existing_call(angles):
    """The list kernel held to dh_fit_identify_subjects_views_device: the step's fitted instances with the fit records of the slots
    that did not want identification marked not-OK give the same dh_ident_record for every slot that did."""
    import torch
    s = main_scene()
    enrolled = np.array([1, 1, 1, 0], np.uint8)
    with pair(angles, "162", 4, s, enrolled=enrolled, sub=dict(retry=0, max_tries=0)) as (tr, ref, got, st, cams, rig, views, model), \
            fit.Fitter() as ftr:
        seen = 0
        for k, (items, present) in enumerate(main_steps(s)[:3]):
            rec = both(tr, ref, s, k, items, present).reshape(-1)
            frec = rec["track"]["fit"].copy()
            frec["status"][rec["identified"] == 0] = fr.FEW_POINTS
            d_frames = torch.from_numpy(s.frames[k].view(np.int16).copy()[None]).cuda()
            out = ftr.identify_subjects_views(d_frames, views, got, to_device(rec["track"]["instance"]), enrolled=to_device(enrolled),
                                              fit_records=to_device(frec), params=fit.ident_views_params(**IDENT), device_out=True)
            torch.cuda.synchronize()
            subjects, irec = out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy().view(_lib.IDENT_RECORD_DTYPE)
            for i in range(len(rec)):
                if rec["identified"][i]:
                    assert irec[i].tobytes() == rec["ident"][i].tobytes(), (k, i, irec[i], rec["ident"][i])
                    assert subjects[i] == rec["subject"][i]
                    seen += 1
                else:
                    assert irec[i]["status"] == ir.SKIPPED == rec["ident"][i]["status"]
        assert seen >= 3


def test_host_calls_against_device_twins_between_guard_bands(angles):
    """The core step, host call against _device twin on a side stream; the twin's records lie between 4 KB guard bands at a pointer
    8 bytes off a 256-byte boundary and nothing outside them changes."""
    import torch
    s = main_scene()
    stream = torch.cuda.Stream()
    nb = s.n_rigs * SLOTS * REC.itemsize
    with pair(angles, "162", 4, s, enrolled=[1, 1, 1, 0], ident=ANY, trackers=2) as ((th, td), ref, *_):
        for k, (items, present) in enumerate(main_steps(s)[:4]):
            want = both(th, ref, s, k, items, present)
            d, mh, d_pr = device_inputs(s, k, items, present)
            buf, ptr, off = guarded(nb, 8)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                step_dev(td, d, mh, ptr, d_pr, stream.cuda_stream)
            stream.synchronize()
            assert untouched(buf, off, nb)
            same_records(buf.cpu().numpy()[off:off + nb].view(REC), want, f"device records of step {k}")
            same_records(td.state(), th.state(), f"device state after step {k}")


def test_reset_and_two_runs_of_one_sequence(angles):
    s = main_scene()
    with pair(angles, "162", 4, s, enrolled=[1, 1, 1, 0], ident=ANY) as (tr, ref, *_):
        first = run_main(tr, ref, s)
        state = tr.state()
        tr.reset(0); ref.reset(0)
        same_records(tr.state(), ref.state, "state after the reset of rig 0")
        assert tr.state()[0].tobytes() == rs.initial(SLOTS).tobytes() and tr.state()[1].tobytes() == state[1].tobytes()
        run_main(tr, ref, s, steps=2)
        tr.reset(); ref.reset()
        assert tr.state().tobytes() == rs.initial((2, SLOTS)).tobytes()
        second = run_main(tr, ref, s)
        assert first.tobytes() == second.tobytes() and tr.state().tobytes() == state.tobytes()
        for rig in (-2, 2):
            with pytest.raises(_lib.DepthheadError, match=f"rig {rig} of 2"):
                tr.reset(rig)


def test_one_step_captured_in_a_graph(angles):
    """The core step's five launches, a linear chain, captured with torch.cuda.graph; each replay is one step and equals the eager step."""
    import torch
    s = sc.scene("162", 3, 96, 96, ((3, (0, sc.STRANGER)), (2, (2,))), 3)
    items = lambda k: [s.item(k, 0, 0, 7), s.item(k, 0, 1, 8), s.item(k, 1, 0, 9)]
    with pair(angles, "162", 3, s, sub=dict(retry=1, max_tries=0), trackers=2) as ((eager, tr), ref, *_):
        d, mh, _ = device_inputs(s, 0, items(0))
        d_rec = torch.zeros(2 * SLOTS * REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step_dev(tr, d, mh, d_rec.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        tr.reset()                                                     # whatever the capture itself ran or did not run
        torch.cuda.synchronize()
        for k in range(3):
            new, _, _ = device_inputs(s, k, items(k))
            for a, b in zip(d, new):
                a.copy_(b)
            g.replay()
            torch.cuda.synchronize()
            want = both(eager, ref, s, k, items(k), what=f"eager step {k}")
            same_records(d_rec.cpu().numpy().view(REC), want, f"replay {k}")
            same_records(tr.state(), eager.state(), f"state after replay {k}")


def test_a_rig_of_one_camera_through_the_identity_is_the_subject_fit_tracker(angles):
    """V = I and u = 0: the world frame is the camera's.  Equal to SubjectFitTracker on the same inputs: the fitted R, t and scale, the
    fit's points, steps, status and sum_r2_fixed, age and lost, the whole dh_ident_record, subject, model, identified and tries of
    every record, and R, t, t_prev, tracked, have_prev, age, lost and the four words of the state."""
    frames, Ks, _, _, poses = sts.sequence("162", 3, 96, 96, (2,), 4)
    sup = fts.good_support(1)
    eye, zero = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)
    ident = dict(min_points=16, max_rms=1e9)
    with gpu_set("162", 3) as (got, st), tracking.Cameras(Ks) as cams, tracking.Rig(cams, eye, zero) as rig, fit.Views(cams, eye, zero) as views, \
            fit.Model(*sts.generic("162")) as model, \
            fit.RigSubjectFitTracker(rig, views, got, model, 96, 96, params=fit.rig_fit_track_params(**TRACK),
                                     ident_params=fit.ident_views_params(**ident)) as tr, \
            fit.SubjectFitTracker(cams, got, model, 96, 96, params=fit.fit_track_params(**TRACK), ident_params=fit.ident_params(**ident)) as single:
        for k in range(4):
            p = np.zeros((1, 16), _lib.RIG_PERSON_DTYPE)
            p[0, 0]["views"], p[0, 0]["n_views"], p[0, 0]["world"], p[0, 0]["id"] = 1, 1, poses[k, 0]["mid_point"], 9
            heads = np.zeros((1, 1), _lib.HEAD_DTYPE)
            heads[0, 0]["pose"] = poses[k, 0]
            a = tr.step_persons(frames[k], [1], heads, [1], p)[0, 0]
            b = single.step_poses(frames[k], poses[k], sup)[0]
            assert a["track"]["status"] == b["track"]["status"] == (ft.CARRIED if k else ft.FITTED), (k, a, b)
            for f in ("R", "t", "scale"):
                assert a["track"]["instance"][f].tobytes() == b["track"]["instance"][f].tobytes(), (k, f)
            assert a["track"]["instance"]["model"] == b["track"]["instance"]["mesh"]
            for f in ("points", "steps", "status", "sum_r2_fixed"):
                assert a["track"]["fit"][f] == b["track"]["fit"][f], (k, f)
            assert (a["track"]["age"], a["track"]["lost"]) == (b["track"]["age"], b["track"]["lost"])
            assert a["ident"].tobytes() == b["ident"].tobytes(), (k, a["ident"], b["ident"])
            for f in ("subject", "model", "identified", "tries"):
                assert a[f] == b[f], (k, f)
        x, y = tr.state()[0, 0], single.state()[0]
        for f in ("R", "t", "t_prev", "tracked", "have_prev", "age", "lost"):
            assert x["fit"][f].tobytes() == y["fit"][f].tobytes(), f
        for f in ("subject", "wait", "tries", "bound_age"):
            assert x[f] == y[f], f
        assert x["subject"] < 3 and x["bound_age"] == 3


def test_one_whole_step_with_a_rig_tracker_on_three_cameras_in_two_rigs(angles):
    """Camera 0 alone, cameras 1 and 2 the rig of two, every camera on the same synthetic frame (the set-up of the rig fit tracker's
    whole-step test).  The whole step's rig outputs equal a RigTracker step of its own on the same frames, and its records the
    restatement's on those outputs; the _device twin gives the same bytes; the second step fits what the first bound with its model."""
    import torch
    from depthhead_amd import prediction, render, synth
    w, h = 128, 112
    rig_begin = [0, 1, 3]
    frames = np.ascontiguousarray(np.broadcast_to(synth.biwi_batch(1, w, h, first=4), (3, h, w)))
    Ks = np.ascontiguousarray(np.broadcast_to(synth.default_intrinsic(w, h), (3, 3, 3)))
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)
    rig_R = np.stack([np.eye(3), np.eye(3), render.euler_to_matrix((0, 20, 0)).astype(np.float64)]).astype(np.float32)
    rig_t = np.zeros((3, 3), np.float32)
    track = dict(keep_points=0, rms_max=4096.0, max_jump=4096.0)          # (a forest's head of a synthetic frame: believe every fit)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(Ks) as cams, gpu_set("162", 3) as (got, st), \
            fit.Model(*sts.generic("162")) as model:
        n0, heads0 = hp.predict_heads_cameras(frames, cams, 4, 30)
        assert n0[1] > 0
        m = heads0[1, 0]["pose"]["mid_point"].astype(np.float64)
        rig_t[2] = m - rig_R[2].astype(np.float64) @ m
        V, u = fit.views_from_rig(rig_R, rig_t)
        ref = rs.Tracker(Ks, V, u, rig_begin, st, sts.generic("162"), angles, scale=0.95, prm=rf.params(**track), ident_prm=ivr.params(**ANY))
        make = lambda: fit.RigSubjectFitTracker(rig, views, got, model, w, h, scale=0.95, params=fit.rig_fit_track_params(**track),
                                                ident_params=fit.ident_views_params(**ANY))
        with tracking.Rig(cams, rig_R, rig_t, rig_begin) as rig, fit.Views(cams, V, u) as views, tracking.RigTracker(hp, rig, w, h) as rt, \
                tracking.RigTracker(hp, rig, w, h) as rt_alone, tracking.RigTracker(hp, rig, w, h) as rt_dev, make() as tr, make() as tr_dev:
            first = None
            for k in range(2):
                outs, rec = tr.step(rt, frames)
                first = rec if first is None else first
                for a, b, what in zip(outs, rt_alone.step(frames), ("n_heads", "heads", "rig_ids", "n_persons", "persons", "tracks")):
                    assert a.tobytes() == b.tobytes(), (k, what)
                n_heads, heads, ids, n_persons, persons, tracks = outs
                assert (n_persons >= 1).all() and (persons["id"][:, 0] != 0).all()
                same_records(rec, ref.step(frames, n_heads, heads, n_persons, persons), f"records of step {k}")
                same_records(tr.state(), ref.state, f"state after step {k}")
                mh = rt.max_heads
                d = {n: torch.zeros(b, dtype=torch.uint8, device="cuda") for n, b in
                     (("n_heads", 3 * 4), ("heads", 3 * mh * 80), ("ids", 3 * mh * 4), ("n_persons", 2 * 4), ("persons", 2 * 16 * 56),
                      ("tracks", 2 * 16 * 72), ("rec", 2 * SLOTS * REC.itemsize))}
                d_frames = to_device(frames)
                tr_dev.step_device(d_frames.data_ptr(), d["n_heads"].data_ptr(), d["heads"].data_ptr(), d["n_persons"].data_ptr(),
                                   d["persons"].data_ptr(), d["rec"].data_ptr(), rig_tracker=rt_dev, ids_ptr=d["ids"].data_ptr(),
                                   tracks_ptr=d["tracks"].data_ptr())
                torch.cuda.synchronize()
                assert d["rec"].cpu().numpy().tobytes() == rec.tobytes() and d["persons"].cpu().numpy().tobytes() == persons.tobytes()
                assert d["heads"].cpu().numpy().tobytes() == heads.tobytes() and d["tracks"].cpu().numpy().tobytes() == tracks.tobytes()
            bound = (first["identified"] == 1) & (first["subject"] != UNKNOWN)
            assert first["identified"].any() and (rec["model"][bound] == first["subject"][bound]).all()
            with tracking.Rig(cams, rig_R, rig_t, rig_begin) as other, tracking.RigTracker(hp, other, w, h) as rt_other:
                with pytest.raises(_lib.DepthheadError, match="another rig table"):
                    tr.step(rt_other, frames)
            with tracking.RigTracker(hp, rig, w, h, max_misses=2) as rt_short:
                with pytest.raises(_lib.DepthheadError, match="max_misses 2 is below the fit tracker's max_coast 3"):
                    tr.step(rt_short, frames)
            same_records(tr.state(), ref.state, "state after the refusals")


def test_refusals_that_need_a_tracker(angles):
    s = sc.scene("162", 3, 96, 96, ((3, (0, 2)),), 2)
    items = [s.item(1, 0, 0, 7), s.item(1, 0, 1, 8)]
    lib, vp = _lib.load(), _lib.vp
    with pair(angles, "162", 3, s, ident=ANY) as (tr, ref, got, st, cams, rig, views, model):
        both(tr, ref, s, 0, [s.item(0, 0, 0, 7), s.item(0, 0, 1, 8)])
        state = tr.state()
        rec = np.full(SLOTS * REC.itemsize, 0xCD, np.uint8)
        n_heads, heads, n_persons, persons = s.inputs(items)
        f = np.ascontiguousarray(s.frames[1])

        def refused(what, fr_=f, w=96, h=96, mh=2, nh=n_heads, hd=heads, npn=n_persons, pn=persons, prm=None, out=rec):
            for name, extra in (("dh_rig_subject_fit_tracker_step_persons", ()), ("dh_rig_subject_fit_tracker_step_persons_device", (None,))):
                rc = getattr(lib, name)(tr._h, vp(fr_), w, h, None, mh, vp(nh), vp(hd), vp(npn), vp(pn), prm, vp(out), *extra)
                msg = lib.dh_last_error().decode()
                assert rc == EINVAL and what in msg and name in msg, (name, rc, msg)
            assert (rec == 0xCD).all()

        refused("NULL frames", fr_=None)
        refused("NULL heads", nh=None); refused("NULL heads", hd=None)
        refused("NULL persons", npn=None); refused("NULL persons", pn=None)
        refused("NULL records", out=None)
        for w, h in ((0, 96), (96, 0), (96, _lib.RENDER_MAX_SIZE + 1)):
            refused("frame size", w=w, h=h)
        refused("max_heads 0 outside 1 .. 4", mh=0); refused("max_heads 5", mh=5)
        for kw, what in ((dict(coarse_iterations=33, iterations=32), "above 64"), (dict(gate=(0.0, 25.0)), "gate[0]"), (dict(min_points=5), "min_points 5 below 6")):
            refused(what, prm=C.byref(fit.fit_params(**kw)))
        for g, rid, subject, what in ((-1, 7, 0, "rig -1"), (1, 7, 0, "rig 1"), (0, 0, 0, "id 0"), (0, 7, 3, "subject 3"), (0, 7, 0xFFFFFFFE, "subject")):
            with pytest.raises(_lib.DepthheadError) as ei:
                tr.bind(g, rid, subject)
            assert ei.value.code == EINVAL and what in str(ei.value)
        assert lib.dh_rig_subject_fit_tracker_state(tr._h, None) == EINVAL and "NULL" in lib.dh_last_error().decode()
        assert lib.dh_rig_subject_fit_tracker_info(tr._h, None, None, None) == 0
        assert tr.state().tobytes() == state.tobytes()                 # nothing was launched
        # ---- creation's refusals past the handles, in the header's order: each with the later faults present too
        h = C.c_void_p(1234)
        wrong = fit.Model(*sts.generic("642"))
        big = float(np.float32(4096.5 / got.info()[4]))
        cams2 = tracking.Cameras(s.Ks)
        views2 = fit.Views(cams2, s.V, s.u)

        def create(what, scale=1.0, ident=None, sub=None, m=model, vw=views, enrolled=None):
            rc = lib.dh_rig_subject_fit_tracker_create(rig._h, vw._h, got._h, m._h, C.c_float(scale), C.c_uint32(0), None, _lib.ref(ident),
                                                       _lib.ref(sub), vp(enrolled), C.byref(h))
            msg = lib.dh_last_error().decode()
            assert rc == EINVAL and what in msg and "dh_rig_subject_fit_tracker_create" in msg and h.value is None, (what, rc, msg)

        bad_sub = _lib.SubjectTrackParams()
        bad_sub.reserved[0] = 1
        create("different camera tables", scale=big, ident=fit.ident_views_params(iterations=65), sub=bad_sub, m=wrong, vw=views2)
        create("iterations = 65 above 64", scale=big, ident=fit.ident_views_params(iterations=65), sub=bad_sub, m=wrong)
        create("min_ratio", scale=big, ident=fit.ident_views_params(min_ratio=0.5), sub=bad_sub, m=wrong)
        create("reserved word of the dh_subject_track_params", scale=big, sub=bad_sub, m=wrong)
        create("the generic model has 642 points, a model of the set 162", scale=big, m=wrong)
        create("a model of the set may span", scale=big)
        create("a model of the set may span", scale=-big)
        wrong.close(); views2.close(); cams2.close()
        far = np.asarray(sts.generic("162")[0]) * np.float32(3.0)         # a generic model larger than the set's bound
        with fit.Model(far, sts.generic("162")[1]) as wide:
            scale = float(np.float32(4096.5 / wide.info()[1]))
            assert scale * got.info()[4] <= 4096.0
            create("the model spans", scale=scale, m=wide)
    # (cameras of the largest rig) * points above DH_FIT_MAX_POINTS, then one pair above DH_IDENT_MAX_PAIRS
    K = np.stack([s.Ks[0]] * 4)
    eye, zero = np.stack([np.eye(3, dtype=np.float32)] * 4), np.zeros((4, 3), np.float32)
    with gpu_set("strip10923", 2) as (long_set, _), tracking.Cameras(K) as cams, tracking.Rig(cams, eye, zero, [0, 3, 4]) as rig, \
            fit.Views(cams, eye, zero) as views, fit.Model(*sts.generic("strip10923")) as strip:
        h = C.c_void_p(1234)
        rc = lib.dh_rig_subject_fit_tracker_create(rig._h, views._h, long_set._h, strip._h, C.c_float(1.0), C.c_uint32(0), None, None, None, None, C.byref(h))
        assert rc == EINVAL and "a rig of 3 cameras sums 32769 terms" in lib.dh_last_error().decode() and h.value is None
    n_rigs = (1 << 22) // (SLOTS * 256) + 1
    K = np.stack([s.Ks[0]] * n_rigs)
    eye, zero = np.stack([np.eye(3, dtype=np.float32)] * n_rigs), np.zeros((n_rigs, 3), np.float32)
    with gpu_set("4", 256) as (big_set, _), tracking.Cameras(K) as many, tracking.Rig(many, eye, zero, list(range(n_rigs + 1))) as rig, \
            fit.Views(many, eye, zero) as views, fit.Model(*sts.generic("4")) as tetra:
        h = C.c_void_p(1234)
        rc = lib.dh_rig_subject_fit_tracker_create(rig._h, views._h, big_set._h, tetra._h, C.c_float(1.0), C.c_uint32(0), None, None, None, None, C.byref(h))
        assert rc == EINVAL and f"{n_rigs} rigs of 16 slots times 256 subjects exceed 4194304 pairs" in lib.dh_last_error().decode() and h.value is None
