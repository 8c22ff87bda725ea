"""The rig fit tracker on the GPU against its restatement (tests/rig_fit_track_ref.py): every field of every
record and of the state after every step, byte for byte -- no tolerance.  The scripts of tests/rig_fit_track_scenes.py through
step_persons on hand-made persons and heads (no forest): detected then carried, the motion flag, an absent camera and an absent
rig, coasting beyond max_coast, an empty frame, an unseen person followed and freed, BAD_JUMP, id 0 / a repeated id / a person
that names no head, two rigs with the second beginning at camera 1, a seventeenth id; the host forms against the _device twins
on a side stream; reset of one rig in mid-sequence; a model of 2562 points (streamed, not staged in LDS); a rig of one camera
through the identity against FitTracker's fit of the same start; one whole step with a real RigTracker on three cameras in
two rigs; two runs of one script byte-identical; the refusals that need a device.  Each restatement run is computed once."""
import ctypes as C
import functools

import numpy as np
import pytest

import fit_ref as fr
import fit_scenes as fs
import fit_track_scenes as fts
import rig_fit_track_ref as rf
import rig_fit_track_scenes as sc
from gpu_kit import guarded, same_records
from depthhead_amd import _lib, fit, render, synth, tracking

pytestmark = pytest.mark.gpu

REC, STATE = _lib.RIG_FIT_RECORD_DTYPE, _lib.RIG_FIT_STATE_DTYPE
SCRIPTS = [("carried", 9000, 0, None), ("carried", 9001, rf.MOTION, 4), ("absent", 9003, rf.MOTION, None), ("coast", 9000, 0, None),
           ("gone", 9001, 0, None), ("unseen", 9002, 0, None), ("jump", 9003, 0, 4), ("unbound", 9000, 0, None),
           ("two_rigs", 9001, rf.MOTION, None), ("full", 9002, 0, None)]


def model_points(kind="head2"):
    v, _, n = fs.head(4 if kind == "2562" else 2)
    return v, n


@pytest.fixture(scope="module")
def gpu():
    angles = fit.angles()
    angles.setflags(write=False)
    with fit.Model(*model_points()) as model:
        yield model, angles


def rig_extrinsics(V, u):
    """The camera-to-world R, t a rig table takes, from the view table's V, u (only rig_begin matters to the fit tracker)."""
    R = np.transpose(np.asarray(V, np.float64), (0, 2, 1))
    return R.astype(np.float32), (-np.einsum("nij,nj->ni", R, np.asarray(u, np.float64))).astype(np.float32)


class Rigged:
    """Cameras, rig table, view table and tracker of a script, closed together."""

    def __init__(self, s, model, **kw):
        self.cams = tracking.Cameras(s["Ks"])
        self.rig = tracking.Rig(self.cams, *rig_extrinsics(s["V"], s["u"]), s["rig_begin"])
        self.views = fit.Views(self.cams, s["V"], s["u"])
        self.tr = fit.RigFitTracker(self.rig, self.views, model, s["w"], s["h"], motion=bool(s["flags"]),
                                    params=fit.rig_fit_track_params(**s["prm"]), **kw)

    def __enter__(self):
        return self.tr

    def __exit__(self, *exc):
        for h in (self.tr, self.views, self.rig, self.cams):
            h.close()


def reference(s, angles, kind="head2"):
    pts, nrm = model_points(kind)
    return rf.Tracker(s["Ks"], s["V"], s["u"], s["rig_begin"], pts, nrm, angles, flags=s["flags"], prm=rf.params(**s["prm"]))


def ref_step(ref, st):
    return ref.step(st["frames"], *st["inputs"], present=st["present"], fit_prm=fr.params(*st["fit"]) if st["fit"] else None)


@functools.lru_cache(maxsize=None)
def ref_run(name, seed, motion, steps):
    """(records [steps, n_rigs, 16], states after every step) of a script in the restatement: computed once."""
    s = sc.script(name, seed, motion)
    ref = reference(s, fit.angles())
    recs, states = [], []
    for st in s["steps"][:steps]:
        recs.append(ref_step(ref, st))
        states.append(ref.state.copy())
    out = np.array(recs), np.array(states)
    for a in out:
        a.setflags(write=False)
    return out


def gpu_step(tr, st):
    return tr.step_persons(st["frames"], *st["inputs"], present=st["present"], fit_params=fit.fit_params(*st["fit"]) if st["fit"] else None)


@pytest.mark.parametrize("name,seed,motion,steps", SCRIPTS, ids=[f"{n}-{m}" for n, _, m, _ in SCRIPTS])
def test_scripts_equal_the_restatement_after_every_step(gpu, name, seed, motion, steps):
    model, _ = gpu
    s = sc.script(name, seed, motion)
    want_rec, want_state = ref_run(name, seed, motion, steps)
    with Rigged(s, model) as tr:
        assert not np.frombuffer(tr.state().tobytes(), np.uint8).any()
        for k, st in enumerate(s["steps"][:steps]):
            got = gpu_step(tr, st)
            assert got.dtype == REC and got.shape == (len(s["rig_begin"]) - 1, 16)
            same_records(got, want_rec[k], f"{name}: records of step {k}")
            same_records(tr.state(), want_state[k], f"{name}: state after step {k}")
    kinds = set((want_rec["status"] & 0xFF).reshape(-1).tolist())
    assert {"carried": {0, 1, 2}, "absent": {0, 1, 2, 4}, "coast": {0, 1, 2, 4}, "gone": {0, 1, 2, 3}}.get(name, kinds) <= kinds


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_host_steps_against_device_twins_between_guard_bands(gpu):
    """The core step, host call against _device twin on a side stream, with an absent camera and an absent rig on the way; the
    twin's records lie between guard bands at an address 8 bytes past a 256-byte boundary."""
    import torch
    model, _ = gpu
    s = sc.script("absent", 9003, rf.MOTION)
    want_rec, want_state = ref_run("absent", 9003, rf.MOTION, None)
    stream = torch.cuda.Stream()
    with Rigged(s, model) as td:
        for k, st in enumerate(s["steps"]):
            n_heads, heads, n_persons, persons = st["inputs"]
            d = [dev(a) for a in (st["frames"], n_heads, heads, n_persons, persons)]
            d_pr = dev(np.asarray(st["present"], np.uint8)) if st["present"] is not None else None
            buf, rec_p, off = guarded(16 * REC.itemsize, skew=8)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                td.step_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), rec_p,
                               max_heads=heads.shape[1], present_ptr=d_pr.data_ptr() if d_pr is not None else 0, stream=stream.cuda_stream)
            stream.synchronize()
            host = buf.cpu().numpy()
            assert (host[:off] == 0xA5).all() and (host[off + 16 * REC.itemsize:] == 0xA5).all()
            same_records(np.frombuffer(host[off:off + 16 * REC.itemsize].tobytes(), REC), want_rec[k], f"device records of step {k}")
            same_records(td.state(), want_state[k], f"device state after step {k}")


def test_reset_of_one_rig_in_mid_sequence(gpu):
    model, angles = gpu
    s = sc.script("two_rigs", 9001, rf.MOTION)
    ref = reference(s, angles)
    with Rigged(s, model) as tr:
        for k, st in enumerate(s["steps"][:5]):
            if k == 2:
                tr.reset(1)
                ref.reset(1)
                assert not np.frombuffer(tr.state().tobytes(), np.uint8).any()
            if k == 3:
                tr.reset(0)                                   # the other rig's reset leaves this one alone
                ref.reset(0)
            got, want = gpu_step(tr, st), ref_step(ref, st)
            same_records(got, want, f"records of step {k}")
            same_records(tr.state(), ref.state, f"state after step {k}")
            if k == 2:
                assert got[1, 0]["status"] == fit.FIT_TRACK_FITTED and got[1, 0]["age"] == 1
        for rig in (2, -2):
            with pytest.raises(_lib.DepthheadError, match=f"rig {rig} of 2"):
                tr.reset(rig)
        tr.reset()
        assert not np.frombuffer(tr.state().tobytes(), np.uint8).any()


def test_a_model_of_2562_points_is_streamed(gpu):
    _, angles = gpu
    s = sc.script("carried", 9002)
    ref = reference(s, angles, "2562")
    assert len(model_points("2562")[0]) == 2562
    with fit.Model(*model_points("2562")) as big, Rigged(s, big) as tr:
        for k, st in enumerate(s["steps"][:2]):
            got, want = gpu_step(tr, st), ref_step(ref, st)
            same_records(got, want, f"records of step {k}")
            same_records(tr.state(), ref.state, f"state after step {k}")
        assert (got[0, 0]["status"], got[0, 0]["age"]) == (fit.FIT_TRACK_CARRIED, 2) and got[0, 0]["fit"]["points"] > 1000


def test_a_rig_of_one_camera_through_the_identity_is_the_fit_tracker(gpu):
    """V = I and u = 0: the world frame is the camera's, the person's world is the pose's mid_point and V^T Rh is Rh, so every
    start, every sum and every output equals FitTracker's, detected and carried, with and without the motion start."""
    model, _ = gpu
    frames, K, pos, Rs, poses = fts.sequence(96, 96, 8002, steps=4)
    sup = fts.good_support()
    eye, zero = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)
    for motion in (False, True):
        with tracking.Cameras(K[None]) as cams, tracking.Rig(cams, eye, zero) as rig, fit.Views(cams, eye, zero) as views, \
                fit.RigFitTracker(rig, views, model, 96, 96, motion=motion) as tr, fit.FitTracker(cams, model, 96, 96, motion=motion) as single:
            for k in range(4):
                p = np.zeros((1, 16), _lib.RIG_PERSON_DTYPE)
                p[0, 0]["views"], p[0, 0]["n_views"], p[0, 0]["world"], p[0, 0]["id"] = 1, 1, poses[k]["mid_point"], 9
                heads = np.zeros((1, 1), _lib.HEAD_DTYPE)
                heads[0, 0]["pose"] = poses[k]
                got = tr.step_persons(frames[k][None], [1], heads, [1], p)[0, 0]
                want = single.step_poses(frames[k][None], poses[k:k + 1], sup)[0]
                assert got["status"] == want["status"] == (fit.FIT_TRACK_CARRIED if k else fit.FIT_TRACK_FITTED), (k, got, want)
                for f in ("R", "t", "scale"):
                    assert got["instance"][f].tobytes() == want["instance"][f].tobytes(), (k, f)
                for f in ("points", "steps", "status", "sum_r2_fixed"):
                    assert got["fit"][f] == want["fit"][f], (k, f)
                assert (got["age"], got["lost"], got["fit"]["views_used"], got["id"], got["person"]) == (want["age"], want["lost"], 1, 9, 0)
            a, b = tr.state()[0, 0], single.state()[0]
            for f in ("R", "t", "t_prev", "tracked", "have_prev", "age", "lost"):
                assert a[f].tobytes() == b[f].tobytes(), f


def test_two_runs_of_one_script_are_byte_identical(gpu):
    model, _ = gpu
    s = sc.script("gone", 9001)
    runs = []
    for _ in range(2):
        with Rigged(s, model) as tr:
            recs = [gpu_step(tr, st).tobytes() for st in s["steps"]]
            runs.append((recs, tr.state().tobytes()))
    assert runs[0] == runs[1]


def test_one_whole_step_with_a_rig_tracker_on_three_cameras_in_two_rigs(gpu):
    """Camera 0 alone, cameras 1 and 2 the rig of two (set up as the last case of test_gpu_fit_views.py: every camera sees the
    same frame, camera 2 is turned 20 degrees about y and placed so that its heaviest head lies on camera 1's in the world).
    The whole step's rig outputs equal a RigTracker step of its own on the same frames, and its records the restatement's on
    those outputs; the _device twin gives the same bytes; the second step carries what the first accepted."""
    import torch
    from depthhead_amd import prediction
    model, angles = gpu
    w, h = 128, 112
    rig_begin = [0, 1, 3]
    frames = np.ascontiguousarray(np.broadcast_to(synth.biwi_batch(1, w, h, first=4), (3, h, w)))
    Ks = np.ascontiguousarray(np.broadcast_to(synth.default_intrinsic(w, h), (3, 3, 3)))
    forest = synth.fit_forest(6, 10, synth.FOREST_SEED_BASE + 9, n_frames=12, subset=1500)
    rig_R = np.stack([np.eye(3), np.eye(3), render.euler_to_matrix((0, 20, 0)).astype(np.float64)]).astype(np.float32)
    rig_t = np.zeros((3, 3), np.float32)
    prm = fit.rig_fit_track_params(keep_points=0, rms_max=4096.0, max_jump=4096.0)     # (a forest's head of a synthetic frame: believe every fit)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(Ks) as cams:
        n0, heads0 = hp.predict_heads_cameras(frames, cams, 4, 30)
        assert n0[1] > 0
        m = heads0[1, 0]["pose"]["mid_point"].astype(np.float64)
        rig_t[2] = m - rig_R[2].astype(np.float64) @ m
        V, u = fit.views_from_rig(rig_R, rig_t)
        ref = rf.Tracker(Ks, V, u, rig_begin, *model_points(), angles, scale=0.95, prm=rf.params(keep_points=0, rms_max=4096.0, max_jump=4096.0))
        with tracking.Rig(cams, rig_R, rig_t, rig_begin) as rig, fit.Views(cams, V, u) as views, \
                tracking.RigTracker(hp, rig, w, h) as rt, tracking.RigTracker(hp, rig, w, h) as rt_alone, \
                tracking.RigTracker(hp, rig, w, h) as rt_dev, \
                fit.RigFitTracker(rig, views, model, w, h, scale=0.95, params=prm) as tr, \
                fit.RigFitTracker(rig, views, model, w, h, scale=0.95, params=prm) as tr_dev:
            first = None
            for k in range(2):
                outs, rec = tr.step(rt, frames)
                first = rec if first is None else first
                alone = rt_alone.step(frames)
                for a, b, what in zip(outs, alone, ("n_heads", "heads", "rig_ids", "n_persons", "persons", "tracks")):
                    assert a.tobytes() == b.tobytes(), (k, what)
                n_heads, heads, ids, n_persons, persons, tracks = outs
                assert (n_persons >= 1).all() and (persons["id"][:, 0] != 0).all()
                same_records(rec, ref.step(frames, n_heads, heads, n_persons, persons), f"records of step {k}")
                same_records(tr.state(), ref.state, f"state after step {k}")
                # the _device twin on device arrays
                mh = rt.max_heads
                d_frames = dev(frames)
                d = {n: torch.zeros(b, dtype=torch.uint8, device="cuda") for n, b in
                     (("n_heads", 3 * 4), ("heads", 3 * mh * 80), ("ids", 3 * mh * 4), ("n_persons", 2 * 4), ("persons", 2 * 16 * 56),
                      ("tracks", 2 * 16 * 72), ("rec", 2 * 16 * REC.itemsize))}
                tr_dev.step_device(d_frames.data_ptr(), d["n_heads"].data_ptr(), d["heads"].data_ptr(), d["n_persons"].data_ptr(),
                                   d["persons"].data_ptr(), d["rec"].data_ptr(), rig_tracker=rt_dev, ids_ptr=d["ids"].data_ptr(),
                                   tracks_ptr=d["tracks"].data_ptr())
                torch.cuda.synchronize()
                assert d["rec"].cpu().numpy().tobytes() == rec.tobytes() and d["persons"].cpu().numpy().tobytes() == persons.tobytes()
                assert d["heads"].cpu().numpy().tobytes() == heads.tobytes() and d["tracks"].cpu().numpy().tobytes() == tracks.tobytes()
            # every slot the first step accepted is carried by the second, under the same id
            accepted = first["status"] == fit.FIT_TRACK_FITTED
            assert accepted.any() and (first["status"][~accepted] & 0xFF != fit.FIT_TRACK_CARRIED).all()
            assert (rec["instance"]["views"][accepted] != 0).all() and (rec["id"][accepted] == first["id"][accepted]).all()
            assert np.isin(rec["status"][accepted] & 0xFF, (fit.FIT_TRACK_CARRIED, fit.FIT_TRACK_REJECTED)).all()
            assert (rec["instance"]["first_cam"][1][rec["status"][1] != 0] == 1).all()
            # the whole step's own refusals
            with tracking.Rig(cams, rig_R, rig_t, rig_begin) as other, tracking.RigTracker(hp, other, w, h) as rt_other:
                with pytest.raises(_lib.DepthheadError, match="another rig table"):
                    tr.step(rt_other, frames)
            with tracking.RigTracker(hp, rig, w, h, max_misses=2) as rt_short:
                with pytest.raises(_lib.DepthheadError, match="max_misses 2 is below the fit tracker's max_coast 3"):
                    tr.step(rt_short, frames)
            same_records(tr.state(), ref.state, "state after the refusals")


def test_refusals_that_need_a_device(gpu):
    model, _ = gpu
    s = sc.script("carried", 9000)
    v4, n4 = model_points("2562")
    reps = -(-10923 // len(v4))
    with tracking.Cameras(s["Ks"]) as cams, tracking.Cameras(s["Ks"]) as cams2, tracking.Rig(cams, *rig_extrinsics(s["V"], s["u"]), [0, 3]) as rig, \
            fit.Views(cams, s["V"], s["u"]) as views, fit.Views(cams2, s["V"], s["u"]) as views2:
        def refused(match, **kw):
            with pytest.raises(_lib.DepthheadError, match=match):
                fit.RigFitTracker(kw.pop("rig", rig), kw.pop("views", views), kw.pop("model", model), 96, 96, **kw)
        refused("different camera tables", views=views2)
        refused("mm from its origin", scale=float(np.float32(4096.5 / model.info()[1])))
        # 3 cameras x 10923 points = 32769 terms: one above the limit; 10922 points pass
        with fit.Model(np.tile(v4, (reps, 1))[:10923], np.tile(n4, (reps, 1))[:10923]) as big, \
                fit.Model(np.tile(v4, (reps, 1))[:10922], np.tile(n4, (reps, 1))[:10922]) as fits:
            refused("a rig of 3 cameras sums 32769 terms", model=big)
            fit.RigFitTracker(rig, views, fits, 96, 96).close()
        with fit.RigFitTracker(rig, views, model, s["w"], s["h"]) as tr:
            st = s["steps"][0]
            n_heads, heads, n_persons, persons = st["inputs"]
            rec = np.full((1, 16), 0, REC)
            rec.view(np.uint8)[:] = 0xCD
            vp = _lib.vp

            def call(frames=st["frames"], w=s["w"], h=s["h"], mh=2, nh=n_heads, hd=heads, npn=n_persons, pn=persons, prm=None, out=rec):
                return tr._lib.dh_rig_fit_tracker_step_persons(tr._h, vp(frames), w, h, None, mh, vp(nh), vp(hd), vp(npn), vp(pn),
                                                               C.byref(prm) if prm is not None else None, vp(out))

            def err():
                return tr._lib.dh_last_error().decode()
            assert call(frames=None) == -1 and "NULL frames" in err()
            assert call(nh=None) == -1 and "NULL heads" in err() and call(hd=None) == -1 and "NULL heads" in err()
            assert call(npn=None) == -1 and "NULL persons" in err() and call(pn=None) == -1 and "NULL persons" in err()
            assert call(out=None) == -1 and "NULL records" in err()
            assert call(w=0) == -1 and "frame size" in err() and call(h=16385) == -1 and "frame size" in err()
            assert call(mh=0) == -1 and "max_heads 0 outside 1 .. 4" in err() and call(mh=5) == -1 and "max_heads 5" in err()
            assert call(prm=fit.fit_params(min_points=5)) == -1 and "min_points 5 below 6" in err()
            assert (rec.view(np.uint8) == 0xCD).all() and not np.frombuffer(tr.state().tobytes(), np.uint8).any()
            assert call() == 0 and (rec[0, 0]["status"], rec[0, 0]["id"]) == (fit.FIT_TRACK_FITTED, 7)
            with pytest.raises(ValueError):
                tr.step_persons(st["frames"][:2], n_heads, heads, n_persons, persons)
