"""The calibration step on the GPU (k_calib_views.hip) against its restatement tests/calib_ref.py: every
byte of every dh_calib_record equal, with no tolerance.  Scenes are those of tests/calib_scenes.py (one head moved through the
volume before three cameras on an arc, several sets); what is compared is the arithmetic, so the instances are true or rough
world poses wherever a fitted one is not what the test is about."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import calib_ref as cr
import calib_scenes as cs
import fit_ref as fr
import fit_scenes as fs
import shape_scenes as ss
import view_fit_scenes as vs
from gpu_kit import fit_models, same_records
from depthhead_amd import _lib, fit, synth
from depthhead_amd.tracking import Cameras

pytestmark = pytest.mark.gpu

INST, REC = _lib.VIEW_INSTANCE_DTYPE, _lib.CALIB_RECORD_DTYPE
GUARD = 4096
SKIP = cr.SKIP
OK, FEW, SINGULAR, NOT_ORTHONORMAL, HELD = fit.CALIB_OK, fit.CALIB_FEW_POINTS, fit.CALIB_SINGULAR, fit.CALIB_NOT_ORTHONORMAL, fit.CALIB_HELD


@functools.lru_cache(maxsize=None)
def host_models():
    """points -> (pts, nrm): head_mesh(2) whole (162), head_mesh(3) whole (642) and its first 63, 255, 256 and 257 points -- a
    wave less one, either side of the workgroup's 256 lanes --, one point that faces the yaw-0 camera, and "flat": 257 points on
    the line y = -x of the plane z = 0 with every normal (0, 0, -1) (test_both_exits)."""
    v2, _, n2 = fs.head(2)
    v3, _, n3 = fs.head(3)
    front = int(np.argmin(v2[:, 2]))
    out = {162: (v2, n2), 642: (v3, n3), 1: (v2[front:front + 1].copy(), n2[front:front + 1].copy())}
    for k in (63, 255, 256, 257):
        out[k] = (v3[:k].copy(), n3[:k].copy())
    x = np.linspace(-1500.0, 1500.0, 257).astype(np.float32)
    out["flat"] = (np.stack([x, -x, np.zeros_like(x)], 1), np.tile(np.array([0.0, 0.0, -1.0], np.float32), (257, 1)))
    return out


@pytest.fixture(scope="module")
def gpu():
    with fit_models(host_models()) as both:
        yield both


@contextlib.contextmanager
def rig(Ks, V, u):
    with Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        yield views


def ref_params(prm):
    return cr.params() if prm is None else cr.params(prm.gate, prm.lam, prm.min_points, tuple(prm.pivot))


def same(got, want, what):
    assert got.dtype == REC
    same_records(got, want, what)


def check(gpu, scene, points, inst, sets=None, take=None, hold=None, prm=None):
    """One host call on model `points` against the restatement.  scene: (frames, Ks, V, u, ...)."""
    ms, ft = gpu
    frames, Ks, V, u = scene[:4]
    pts, nrm = host_models()[points]
    with rig(Ks, V, u) as views:
        got = ft.calibrate_step(frames, views, ms[points], inst, sets=sets, take=take, hold=hold, params=prm)
    want = cr.calib_step(frames, Ks, V, u, pts, nrm, inst, sets, take, hold, ref_params(prm))
    same(got, want, "record")
    return got


@functools.lru_cache(maxsize=None)
def rig_instances(seed=0, n_sets=2, w=160, h=120):
    """(scene with a table a little OFF the true one, instances [2 * n_sets], sets): the true world poses, then rough starts, three views each."""
    frames, Ks, Vt, ut, pos, Rs = cs.rig(seed, n_sets, w, h)
    V, u = off_table(Vt, ut, seed)
    inst = cs.as_records(cs.true_instances(pos, Rs) + cs.rough_instances(seed, pos, Rs))
    inst["flags"] = 0x5A0000 + np.arange(len(inst))      # ignored by the step
    inst["model"][1::2] = 7                              # ignored too: a call has one model
    inst.setflags(write=False)
    sets = np.tile(np.arange(n_sets, dtype=np.uint32), 2)
    sets.setflags(write=False)
    return (frames, Ks, V, u, pos, Rs), inst, sets


def off_table(Vt, ut, seed, off_mm=8.0, off_deg=1.0):
    """A table a little off the true one in every camera (seeded), rounded to f32 once."""
    V, u = Vt.astype(np.float64), ut.astype(np.float64)
    rng = synth.SplitMix(990000 + seed)
    for c in range(len(V)):
        uu = rng.uniform(6)
        Cm = fit.euler_to_matrix(off_deg * (2.0 * uu[:3] - 1.0)).astype(np.float64)
        V[c], u[c] = Cm @ V[c], Cm @ u[c] + off_mm * (2.0 * uu[3:] - 1.0)
    return vs._ro(V.astype(np.float32), u.astype(np.float32))


def test_one_instance_one_identity_view_sums_what_the_fit_sums(gpu):
    """V = I, u = 0, the pivot at t: the record's points and sum_r2_fixed are those of the single-view fit's last pass at the same
    pose (a fit of no steps)."""
    ms, ft = gpu
    frame, K, pos, R = fs.scene(96, 96, 7100)
    eye, zero = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)
    world = cs.as_records([{"first_cam": 0, "views": 1, "R": R, "t": pos, "scale": 1.0}])
    prm = fit.calib_params(min_points=16, pivot=np.float32(pos))
    rec = check(gpu, (frame[None, None], K[None], eye, zero), 162, world, prm=prm)
    assert rec["status"][0] == OK and rec["points"][0] >= 30 and rec["pairs"][0] == 1 and rec["delta"][0].any()
    single = np.zeros(1, _lib.RENDER_INSTANCE_DTYPE)
    single[0] = (0, 0, np.float32(R).reshape(9), np.float32(pos), 1.0, 0)
    _, frec = ft.fit(frame[None], [ms[162]], single, K, params=fit.fit_params(coarse_iterations=0, iterations=0))
    assert (frec["points"][0], frec["sum_r2_fixed"][0]) == (rec["points"][0], rec["sum_r2_fixed"][0])


@pytest.mark.parametrize("points", (1, 63, 255, 256, 257, 642))
def test_model_sizes(gpu, points):
    scene, inst, sets = rig_instances()
    rec = check(gpu, scene, points, inst, sets, prm=fit.calib_params(min_points=1))
    assert (rec["points"] > 0).all() and set(rec["status"].tolist()) <= {OK, SINGULAR, NOT_ORTHONORMAL}
    if points == 642:
        assert (rec["status"] == OK).all() and (rec["points"] > 4 * 150).all() and rec["pairs"].tolist() == [4, 4, 4]


@functools.lru_cache(maxsize=None)
def wide_rig(n, w=96, h=96):
    """A table of n cameras: the three of a rig over and over (camera c is camera c mod 3, with its frame), a little off."""
    frames, Ks, Vt, ut, pos, Rs = cs.rig(3, 1, w, h)
    V, u = off_table(Vt, ut, 3)
    pick = np.arange(n) % 3
    return vs._ro(np.ascontiguousarray(frames[:, pick]), np.ascontiguousarray(Ks[pick]), np.ascontiguousarray(V[pick]),
                  np.ascontiguousarray(u[pick]), pos, Rs)


def world(scene, first_cam, views, s=0):
    return {"first_cam": first_cam, "views": views, "R": np.float32(scene[5][s]), "t": np.float32(scene[4][s]), "scale": np.float32(1.0)}


def test_masks_with_gaps_a_single_high_bit_and_first_cam_above_zero(gpu):
    scene = wide_rig(9)
    items = [world(scene, 0, 0b101), world(scene, 3, 1 << 5), world(scene, 2, 0b1010001), world(scene, 8, 1)]
    rec = check(gpu, scene, 162, cs.as_records(items), prm=fit.calib_params(min_points=16))
    # cameras: 0 and 2; 8; 2, 6 and 8; 8
    assert rec["pairs"].tolist() == [1, 0, 2, 0, 0, 0, 1, 0, 3]
    assert [s == OK for s in rec["status"]] == [p > 0 for p in rec["pairs"]] and (rec["status"][rec["pairs"] == 0] == FEW).all()


@pytest.mark.parametrize("n, first_cam", ((64, 0), (70, 6)))
def test_all_64_bits(gpu, n, first_cam):
    """64 views of one instance: every rank of the grid is busy; in a table of 70 cameras the ranks are fewer than the cameras."""
    scene = wide_rig(n)
    mask = (1 << 64) - 1
    rec = check(gpu, scene, 63, cs.as_records([world(scene, first_cam, mask), world(scene, first_cam, 0b11)]), prm=fit.calib_params(min_points=1))
    want_pairs = [0] * first_cam + [2, 2] + [1] * 62 + [0] * (n - first_cam - 64)
    assert rec["pairs"].tolist() == want_pairs and (rec["points"][first_cam:first_cam + 64] > 0).all()
    assert (rec["status"][:first_cam] == FEW).all()


def test_a_table_of_one_camera(gpu):
    scene = wide_rig(1)
    rec = check(gpu, scene, 162, cs.as_records([world(scene, 0, 1), world(scene, 0, 1)]), prm=fit.calib_params(min_points=16))
    assert rec["pairs"][0] == 2 and rec["status"][0] == OK and len(rec) == 1


def test_three_sets_in_mixed_order_and_no_sets(gpu):
    scene, inst, _ = rig_instances(1, 3)
    mixed = np.array([2, 0, 1, 1, 2, 0], np.uint32)
    six = inst[[2, 0, 1, 4, 5, 3]]
    rec = check(gpu, scene, 162, six, mixed)
    assert rec["pairs"].tolist() == [6, 6, 6] and (rec["status"] == OK).all()
    same(check(gpu, scene, 162, six[::-1].copy(), mixed[::-1].copy()), rec, "the order of the instances is free")
    first = check(gpu, scene, 162, inst[[0, 3]], prm=fit.calib_params(min_points=16))                   # sets = None: set 0
    same(check(gpu, scene, 162, inst[[0, 3]], np.zeros(2, np.uint32), prm=fit.calib_params(min_points=16)), first, "sets = None is set 0")
    same(check(gpu, (scene[0][:1],) + scene[1:], 162, inst[[0, 3]], prm=fit.calib_params(min_points=16)), first, "and the frames of one set alone")


def beyond_the_arm(scene, item, cam, axis=2, by=2050.0):
    """`item` moved so that its pair with camera `cam` lies `by` mm from the camera's pivot (the origin's image) along `axis`."""
    V, u = scene[2][cam].astype(np.float64), scene[3][cam].astype(np.float64)
    off = np.zeros(3)
    off[axis] = by
    out = dict(item)
    out["t"] = (V.T @ off).astype(np.float32)                             # t_v - g_c = V t_w
    return out


def test_twelve_instances_with_an_empty_view_two_skipped_and_one_beyond_the_arm(gpu):
    scene, inst, sets = rig_instances(0, 3)
    frames = scene[0].copy()
    frames[1, 2] = 0                                                  # camera 2 sees nothing at set 1
    scene = (frames,) + scene[1:]
    twelve = inst[np.arange(12) % 6].copy()
    twelve["t"][6:, 0] += np.float32(3.0)
    st = sets[np.arange(12) % 6].copy()
    take = np.array([0, 0, 2, SKIP, 2, 2, 0, 0, SKIP, 2, 0, 2], np.uint32)
    twelve[11] = cs.as_records([beyond_the_arm(scene, world(scene, 0, 0b111), 0)])[0]
    rec = check(gpu, scene, 162, twelve, st, take)
    # ten take part; instances 1, 4, 7 and 10 are in set 1, where camera 2 is blank; instance 11 is beyond camera 0's arm (and
    # passes no point elsewhere: its head is far from where the frames show one)
    assert rec["pairs"].tolist() == [9, 9, 5] and (rec["status"] == OK).all()
    keep = take != SKIP
    same(check(gpu, scene, 162, twelve[keep], st[keep], take[keep]), rec, "without the skipped")
    same(check(gpu, scene, 162, twelve[keep][:-1], st[keep][:-1]), rec, "without the one beyond the arm, take = NULL")
    junk = twelve.copy()
    junk["t"][3] = (1e30, np.nan, 0.0); junk["first_cam"][8] = 4000; junk["R"][8] = np.inf; junk["views"][3] = 0
    ms, ft = gpu
    with rig(*scene[1:4]) as views:
        same(ft.calibrate_step(frames, views, ms[162], junk, sets=st, take=take), rec, "junk in the skipped")


@functools.lru_cache(maxsize=None)
def many(count):
    """`count` (instance, view) pairs, all of camera 0: the rig's true poses at two sets, each moved by a few seeded millimetres."""
    scene, inst, sets = rig_instances()
    out = inst[np.arange(count) % 2].copy()
    out["views"] = 1
    out["t"] += (6.0 * synth.SplitMix(4243).uniform(3 * count).reshape(count, 3) - 3.0).astype(np.float32)
    out.setflags(write=False)
    return scene, out, np.ascontiguousarray(sets[np.arange(count) % 2])


@pytest.mark.parametrize("count", (1, 255, 257))
def test_pair_counts_into_one_row(gpu, count):
    scene, inst, sets = many(count)
    rec = check(gpu, scene, 162, inst, sets, prm=fit.calib_params(min_points=16))
    assert rec["status"].tolist() == [OK, FEW, FEW] and rec["pairs"].tolist() == [count, 0, 0] and rec["points"][0] > 30 * count


def test_held_cameras(gpu):
    scene, inst, sets = rig_instances()
    free = check(gpu, scene, 162, inst, sets)
    for hold in ([0, 1, 0], [1, 0, 7], [1, 1, 1], [0, 0, 0]):
        hd = np.array(hold, np.uint8)
        rec = check(gpu, scene, 162, inst, sets, hold=hd)
        for c in range(3):
            if hold[c]:
                assert rec["status"][c] == HELD and rec["points"][c] == 0 and rec["pairs"][c] == 0 and rec["sum_r2_fixed"][c] == 0
                assert rec["V"][c].tobytes() == scene[2][c].tobytes() and rec["u"][c].tobytes() == scene[3][c].tobytes() and not rec["delta"][c].any()
            else:
                assert rec[c].tobytes() == free[c].tobytes() and rec["status"][c] == OK            # cameras do not touch one another


def test_a_pivot_that_is_not_the_origin(gpu):
    scene, inst, sets = rig_instances()
    at_origin = check(gpu, scene, 162, inst, sets)
    pivot = scene[4].mean(axis=0)
    moved = check(gpu, scene, 162, inst, sets, prm=fit.calib_params(pivot=pivot))
    far = check(gpu, scene, 162, inst, sets, prm=fit.calib_params(pivot=(300.0, -200.0, 500.0)))
    # the sums that do not hold the pivot are the same; the step is another
    for rec in (moved, far):
        assert rec["points"].tolist() == at_origin["points"].tolist() and rec["sum_r2_fixed"].tolist() == at_origin["sum_r2_fixed"].tolist()
        assert (rec["status"] == OK).all() and rec["delta"].tobytes() != at_origin["delta"].tobytes()
    # a pivot so far that every pair is beyond the arm
    none = check(gpu, scene, 162, inst, sets, prm=fit.calib_params(pivot=(0.0, 0.0, 5000.0)))
    assert (none["status"] == FEW).all() and not none["points"].any() and not none["pairs"].any()


def test_gates_and_min_points(gpu):
    scene, inst, sets = rig_instances()
    narrow = check(gpu, scene, 162, inst, sets, prm=fit.calib_params(gate=1.0, min_points=1))
    wide = check(gpu, scene, 162, inst, sets, prm=fit.calib_params(gate=256.0))
    usual = check(gpu, scene, 162, inst, sets)
    assert (0 < narrow["points"]).all() and (narrow["points"] < usual["points"]).all() and (usual["points"] < wide["points"]).all()
    count = int(usual["points"].min())
    c = int(usual["points"].argmin())
    at = check(gpu, scene, 162, inst, sets, prm=fit.calib_params(min_points=count))
    above = check(gpu, scene, 162, inst, sets, prm=fit.calib_params(min_points=count + 1))
    assert at.tobytes() == usual.tobytes()
    assert above["status"][c] == FEW and not above["delta"][c].any()
    assert above["V"][c].tobytes() == scene[2][c].tobytes() and above["u"][c].tobytes() == scene[3][c].tobytes()
    assert (above["points"][c], above["pairs"][c], above["sum_r2_fixed"][c]) == (count, 4, usual["sum_r2_fixed"][c])


@functools.lru_cache(maxsize=None)
def flat_scene(count=400):
    """One camera at the identity looking at a wall 4000 mm away, and `count` copies of the "flat" model lying in it."""
    frames = np.full((1, 1, 120, 160), 4000, np.uint16)
    Ks = np.ascontiguousarray(synth.default_intrinsic(160, 120), np.float32)[None]
    inst = cs.as_records([{"first_cam": 0, "views": 1, "R": np.eye(3, dtype=np.float32), "t": np.array([0, 0, 4000], np.float32), "scale": 1.0}] * count)
    return vs._ro(frames, Ks, np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)), inst


def test_both_exits(gpu):
    """FEW_POINTS: empty frames.  SINGULAR: the 1e-9 on the diagonal keeps a zero column's pivot positive, so a zero pivot needs
    section 20's case -- two identical columns whose diagonal has grown to 2^24, where a + 1e-9 == a, with lambda = 0: the
    second's pivot is a - (a / a) * a = 0.  The "flat" model gives it: every normal is (0, 0, -1) and every point has y = -x, so
    about a pivot on the axis J_3 = -q_1 / 64 and J_4 = q_0 / 64 are the same number; 400 pairs sum (x / 64)^2 past 2^24.  With
    the default lambda, and with 40 pairs, the same scene goes on."""
    scene, inst = flat_scene()
    prm = fit.calib_params(lam=0.0, pivot=(0.0, 0.0, 4000.0))
    empty = check(gpu, (np.zeros_like(scene[0]),) + scene[1:], "flat", inst, prm=prm)
    assert (empty["status"][0], empty["points"][0], empty["pairs"][0], empty["sum_r2_fixed"][0]) == (FEW, 0, 0, 0)
    got = check(gpu, scene, "flat", inst, prm=prm)
    assert got["status"][0] == SINGULAR and not got["delta"].any() and got["points"][0] == 400 * 257 and got["pairs"][0] == 400
    assert got["V"][0].tobytes() == scene[2][0].tobytes() and got["u"][0].tobytes() == scene[3][0].tobytes()
    assert check(gpu, scene, "flat", inst, prm=fit.calib_params(pivot=(0.0, 0.0, 4000.0)))["status"][0] == OK
    assert check(gpu, scene, "flat", inst[:40], prm=prm)["status"][0] == OK


@functools.lru_cache(maxsize=None)
def tolerance_edge():
    """status -> (V, u, camera): tables of rig_instances()'s cameras, each a seeded table a little off the true one with ONE camera
    scaled by the largest factor (walking down from sqrt(1 + DH_FIT_VIEW_TOLERANCE) in steps of 3e-8) that dh_fit_views_create
    still takes.  The turn of the step, rounded to f32, leaves one such camera within the tolerance and pushes another out of
    it: the first of each kind over the table seeds 0 .. 39, found with the restatement."""
    scene, inst, sets = rig_instances()
    frames, Ks = scene[:2]
    Vt, ut = cs.rig(0, 2)[2:4]
    pts, nrm = host_models()[162]
    found = {}
    for k in range(40):
        V, u = off_table(Vt, ut, k)
        for cam in range(3):
            s = np.sqrt(1.001) + 2e-7
            while True:
                Vs = V.copy()
                Vs[cam] = (s * V[cam].astype(np.float64)).astype(np.float32)
                if cr._gram_within(Vs[cam].astype(np.float64), cr.VIEW_TOLERANCE):
                    break
                s -= 3e-8
            hold = np.ones(3, np.uint8)
            hold[cam] = 0
            status = int(cr.calib_step(frames, Ks, Vs, u, pts, nrm, inst, sets, None, hold)["status"][cam])
            found.setdefault(status, (Vs, u, cam))
            if OK in found and NOT_ORTHONORMAL in found:
                return found
    return found


def test_not_orthonormal_at_the_tolerance_edge(gpu):
    scene, inst, sets = rig_instances()
    found = tolerance_edge()
    assert set(found) == {OK, NOT_ORTHONORMAL}
    for status, (Vs, u, cam) in found.items():
        hold = np.ones(3, np.uint8)
        hold[cam] = 0
        rec = check(gpu, (scene[0], scene[1], Vs, u), 162, inst, sets, hold=hold)
        assert rec["status"].tolist() == [status if c == cam else HELD for c in range(3)]
        assert rec["points"][cam] > 64 and rec["pairs"][cam] == 4
        if status == NOT_ORTHONORMAL:
            assert rec["V"][cam].tobytes() == Vs[cam].tobytes() and rec["u"][cam].tobytes() == u[cam].tobytes() and not rec["delta"][cam].any()
        else:
            assert rec["V"][cam].tobytes() != Vs[cam].tobytes() and rec["delta"][cam].all()


def device_step(ft, views, model, d_frames, inst, sets=None, take=None, hold=None, prm=None, stream=None):
    """The _device form on host arrays copied to the device; the records back on the host."""
    import torch
    d_inst = torch.from_numpy(np.ascontiguousarray(inst).view(np.uint8).copy()).cuda()
    d_sets = None if sets is None else torch.from_numpy(np.ascontiguousarray(sets, np.uint32).view(np.int32).copy()).cuda()
    d_take = None if take is None else torch.from_numpy(np.ascontiguousarray(take, np.uint32).view(np.int32).copy()).cuda()
    d_hold = None if hold is None else torch.from_numpy(np.ascontiguousarray(hold, np.uint8).copy()).cuda()
    rec = ft.calibrate_step(d_frames, views, model, d_inst, sets=d_sets, take=d_take, hold=d_hold, params=prm, device_out=True, stream=stream)
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(REC)


BAD = ("no view", "a bit beyond n", "a set beyond n_sets", "a NaN in R", "an R that is no rotation", "beyond the extent")


@pytest.mark.parametrize("which", range(len(BAD)))
def test_the_device_skips_an_instance_the_host_form_refuses(gpu, which):
    """One bad instance among good neighbours: the device leaves it out as a whole, the records equal a run without it, and the
    host form refuses the call."""
    import torch
    ms, ft = gpu
    scene, inst, sets = rig_instances()
    frames, Ks, V, u = scene[:4]
    pts, nrm = host_models()[162]
    bad, st = inst.copy(), sets.copy()
    radius = ms[162].info()[1]
    refusal = ["is seen by no view", "names camera 3 of 3", "names set 2 of 2", "has a non-finite R, t or scale", "not orthonormal",
               "mm from its origin"][which]
    if which == 0:
        bad["views"][1] = 0
    elif which == 1:
        bad["views"][1] = 0b1011
    elif which == 2:
        st[1] = 2
    elif which == 3:
        bad["R"][1, 5] = np.nan
    elif which == 4:
        bad["R"][1, 1] += np.float32(0.2)
    else:
        bad["scale"][1] = np.float32(4100.0 / radius)
    with rig(Ks, V, u) as views:
        with pytest.raises(_lib.DepthheadError) as ei:
            ft.calibrate_step(frames, views, ms[162], bad, sets=st)
        assert ei.value.code == -1 and "instance 1 " in str(ei.value) and refusal in str(ei.value), str(ei.value)
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        got = device_step(ft, views, ms[162], d_frames, bad, st)
        good = device_step(ft, views, ms[162], d_frames, inst, sets)
    without = np.array([0, SKIP, 0, 0], np.uint32)
    same(got, cr.calib_step(frames, Ks, V, u, pts, nrm, inst, sets, without), BAD[which])
    same(got, cr.calib_step(frames, Ks, V, u, pts, nrm, bad, st), "the restated skip")
    assert got["pairs"].tolist() == [3, 3, 3] and good["pairs"].tolist() == [4, 4, 4]


def test_device_twin_chained_after_a_device_fit(gpu):
    """dh_fit_depth_views_device, then dh_fit_calibrate_views_device on its `out`, on a side stream with no host copy or wait
    between them; the records lie between 4 KB guard bands at a pointer that is 8 bytes off a 256-byte line."""
    import torch
    ms, ft = gpu
    frames, Ks, Vt, ut, pos, Rs = cs.rig(2, 1)
    V, u = off_table(Vt, ut, 2)
    pts, nrm = host_models()[162]
    starts = cs.as_records(cs.rough_instances(2, pos, Rs) + cs.rough_instances(3, pos, Rs, 10.0, 4.0) + cs.rough_instances(4, pos, Rs, 20.0, 5.0))
    starts["views"] = (0b111, 0b011, 0b110)
    take = np.array([0, SKIP, 5], np.uint32)
    hold = np.array([0, 1, 0], np.uint8)
    prm = fit.calib_params(min_points=16, pivot=pos[0])
    bytes_ = 3 * REC.itemsize
    stream = torch.cuda.Stream()
    with rig(Ks, V, u) as views:
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_take = torch.from_numpy(take.view(np.int32).copy()).cuda()
        d_hold = torch.from_numpy(hold.copy()).cuda()
        buf = torch.full((GUARD + 8 + bytes_ + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            d_out, d_rec = ft.fit_views(d_frames[0], [ms[162]], starts, views, device_out=True, stream=stream.cuda_stream)
            _lib.check(ft._lib.dh_fit_calibrate_views_device(
                ft._h, C.c_void_p(d_frames.data_ptr()), C.c_uint32(1), 160, 120, views._h, ms[162]._h, C.c_void_p(d_out.data_ptr()),
                C.c_uint32(3), None, C.c_void_p(d_take.data_ptr()), C.c_void_p(d_hold.data_ptr()), C.byref(prm),
                C.c_void_p(buf.data_ptr() + GUARD + 8), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        fitted = d_out.cpu().numpy().view(INST)
        status = d_rec.cpu().numpy().view(_lib.VIEW_FIT_RECORD_DTYPE)["status"]
        host = ft.calibrate_step(frames, views, ms[162], fitted, take=take, hold=hold, params=prm)
    want = cr.calib_step(frames, Ks, V, u, pts, nrm, fitted, None, take, hold, ref_params(prm))
    same(host, want, "host form on the fitted instances")
    raw = buf.cpu().numpy()
    assert (raw[:GUARD + 8] == 0xEE).all() and (raw[GUARD + 8 + bytes_:] == 0xEE).all()
    same(raw[GUARD + 8:GUARD + 8 + bytes_].copy().view(REC), want, "device form")
    assert (status == fit.FIT_OK).all() and want["status"].tolist() == [OK, HELD, OK] and want["pairs"].tolist() == [1, 0, 2]


def test_a_fitter_reused_and_the_other_calls_unchanged(gpu):
    """A smaller, a larger and an empty calibration call, twice over, on a fitter that also fits and takes both shape steps:
    Fitter.fit_views, Fitter.shape_step and Fitter.shape_step_views give the same bytes before and after."""
    ms, _ = gpu
    scene, inst, sets = rig_instances(0, 3)
    frames, Ks, V, u = scene[:4]
    pts, nrm = host_models()[162]
    B = synth.head_basis(np.asarray(pts, np.float64)).astype(np.float32)
    small_scene = wide_rig(1)
    small = cs.as_records([world(small_scene, 0, 1)])
    prm = fit.calib_params(min_points=16)
    want_small = cr.calib_step(*small_scene[:4], pts, nrm, small, prm=ref_params(prm))
    want_large = cr.calib_step(frames, Ks, V, u, pts, nrm, inst, sets, None, [0, 1, 0], ref_params(prm))
    R1, t1 = vs.camera_pose(V[1], u[1], scene[5][0], scene[4][0])
    single = ss.as_records([{"frame": 0, "R": R1, "t": t1, "scale": np.float32(1.0)}])
    starts = inst[3:4].copy()
    starts["model"] = 0
    sprm = fit.shape_params(min_points=16)
    with fit.Fitter() as ft, fit.ShapeBasis(B) as sb, rig(Ks, V, u) as views, rig(*small_scene[1:4]) as small_views:
        def others():
            a = ft.fit_views(frames[0], [ms[162]], starts, views)
            b = ft.shape_step(frames[0, 1:2], ms[162], sb, single, Ks[1], params=sprm)
            c = ft.shape_step_views(frames, views, ms[162], sb, inst, sets=sets, params=sprm)
            return a[0].tobytes(), a[1].tobytes(), b.tobytes(), c.tobytes()
        before = others()
        for _ in range(2):
            same(ft.calibrate_step(small_scene[0], small_views, ms[162], small, params=prm), want_small, "small")
            same(ft.calibrate_step(frames, views, ms[162], inst, sets=sets, hold=[0, 1, 0], params=prm), want_large, "large")
            mid = others()
        none = ft.calibrate_step(frames, views, ms[162], inst[:0], hold=[0, 1, 0])
        assert none["status"].tolist() == [FEW, HELD, FEW] and not none["points"].any() and not none["delta"].any()
        same(none, cr.calib_step(frames, Ks, V, u, pts, nrm, inst[:0], hold=[0, 1, 0]), "empty call")
        after = others()
    assert before == mid == after
    assert np.frombuffer(before[3], _lib.SHAPE_RECORD_DTYPE)["points"][0] > 16


def test_two_runs_are_byte_identical(gpu):
    scene, inst, sets = many(255)
    spread = inst.copy()
    spread["views"] = np.uint64(1) << (np.arange(255) % 3).astype(np.uint64)
    a = check(gpu, scene, 642, spread, sets)
    b = check(gpu, scene, 642, spread, sets)
    assert a.tobytes() == b.tobytes() and (a["status"] == OK).all() and a["pairs"].tolist() == [85, 85, 85]


def test_calibrate_views_is_the_restated_driver(gpu):
    """fit.calibrate_views -- a short schedule: two steps, one wide, one round of one joint step -- on three sets at 80 x 60
    against calib_ref.calibrate_views: the table, the instances and every record of the trace to the bit."""
    ms, ft = gpu
    frames, Ks, Vt, ut, pos, Rs = cs.rig(5, 3, 80, 60)
    V0, u0 = off_table(Vt, ut, 5)
    pts, nrm = host_models()[162]
    starts = cs.rough_instances(5, pos, Rs)
    kw = dict(steps=2, wide_steps=1, rounds=1, joint_steps=1, min_points=32)
    with Cameras(Ks) as cams:
        V, u, inst, trace = fit.calibrate_views(ft, frames, cams, V0, u0, ms[162], cs.as_records(starts), sets=[0, 1, 2], hold=cs.HOLD, **kw)
    wV, wu, winst, wtrace = cr.calibrate_views(frames, Ks, V0, u0, pts, nrm, starts, [0, 1, 2], cs.HOLD, **kw)
    assert V.tobytes() == wV.tobytes() and u.tobytes() == wu.tobytes() and len(trace) == len(wtrace) == 3
    assert inst.tobytes() == cs.as_records(winst).tobytes()
    for got, want in zip(trace, wtrace):
        assert got["stage"] == want["stage"]
        same(got["records"], want["records"], got["stage"])
        assert got["fit"]["status"].tolist() == [r["status"] for r in want["fit"]]
        assert got["fit"]["points"].tolist() == [r["points"] for r in want["fit"]]
    assert [t["stage"] for t in trace] == ["held", "held", "joint 0"]
    assert trace[-1]["records"]["status"].tolist() == [OK, HELD, OK]
    assert V[cs.MIDDLE].tobytes() == V0[cs.MIDDLE].tobytes()


def test_views_from_records(gpu):
    scene, inst, sets = rig_instances()
    frames, Ks, V, u = scene[:4]
    rec = check(gpu, scene, 162, inst, sets, hold=np.array([0, 1, 0], np.uint8))
    rec = rec.copy()
    rec["status"][2] = FEW                                             # as if camera 2 had seen too little
    with Cameras(Ks) as cams, fit.views_from_records(cams, V, u, rec) as nxt:
        assert nxt.info()[0] == 3
        assert nxt.V[0].tobytes() == rec["V"][0].tobytes() and nxt.u[0].tobytes() == rec["u"][0].tobytes()
        assert nxt.V[0].tobytes() != V[0].tobytes()
        for c in (1, 2):
            assert nxt.V[c].tobytes() == V[c].tobytes() and nxt.u[c].tobytes() == u[c].tobytes()
        with pytest.raises(ValueError):
            fit.views_from_records(cams, V, u, rec[:2])


def test_refusals_that_need_a_model(gpu):
    import torch
    ms, ft = gpu
    scene, inst, sets = rig_instances()
    frames, Ks, V, u = scene[:4]

    def refused(what, fn):
        with pytest.raises(_lib.DepthheadError) as ei:
            fn()
        assert ei.value.code == -1 and what in str(ei.value) and "dh_fit_calibrate_views" in str(ei.value), str(ei.value)

    with rig(Ks, V, u) as views:
        radius = ms[162].info()[1]
        over = inst[:1].copy()
        for scale in (float(np.float32(4100.0 / radius)), -float(np.float32(4100.0 / radius))):
            over["scale"] = scale
            refused("mm from its origin", lambda: ft.calibrate_step(frames, views, ms[162], over))
        # 2^23 terms: 13067 pairs of 642 points into one camera.  One pair more passes the count with that camera held, or spread
        # over the cameras, and is refused for the NEXT reason (the last instance names a set that does not exist) before
        # anything runs; so do 13066 pairs and that instance.
        more = np.repeat(inst[:1], 13068)
        more["views"] = 0b100
        refused("camera 2 has more than 8388608 terms", lambda: ft.calibrate_step(frames, views, ms[642], more[:13067]))
        st = np.zeros(13068, np.uint32)
        st[-1] = 2
        refused("camera 2 has more than 8388608 terms", lambda: ft.calibrate_step(frames, views, ms[642], more, sets=st))
        refused("instance 13067 names set 2 of 2", lambda: ft.calibrate_step(frames, views, ms[642], more, sets=st, hold=[0, 0, 1]))
        refused("instance 13066 names set 2 of 2", lambda: ft.calibrate_step(frames, views, ms[642], more[:13067], sets=st[-13067:]))
        spread = more.copy()
        spread["views"] = np.uint64(1) << (np.arange(13068) % 3).astype(np.uint64)
        refused("instance 13067 names set 2 of 2", lambda: ft.calibrate_step(frames, views, ms[642], spread, sets=st))
        spread = spread[:13067]
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        d_lots = torch.from_numpy(spread.view(np.uint8).copy()).cuda()
        refused("13067 instances of 642 points exceed", lambda: ft.calibrate_step(d_frames, views, ms[642], d_lots, device_out=True))
        with pytest.raises(ValueError):
            ft.calibrate_step(frames[:, :2], views, ms[162], inst)
