"""Identifying enrolled subjects across the views of a rig on the GPU (k_ident_views.hip) against its
restatement tests/ident_views_ref.py: subjects, records, poses and every pair's 32-byte score equal as bytes, with no tolerance.
Frames are splatted per camera from a subject's own model (tests/ident_views_scenes.py), 96x96 or 160x120 (48x48 for the table of
34 cameras), so a case costs little at any mesh size."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import fit_ref as fr
import ident_ref as ir
import ident_views_ref as ivr
import ident_views_scenes as ivs
import shape_scenes as ss
import shape_views_scenes as svs
from gpu_kit import to_device
from depthhead_amd import _lib, fit
from depthhead_amd.tracking import Cameras

pytestmark = pytest.mark.gpu

INST, REC, FREC, SCORE1 = _lib.VIEW_INSTANCE_DTYPE, _lib.IDENT_RECORD_DTYPE, _lib.VIEW_FIT_RECORD_DTYPE, _lib.FIT_RECORD_DTYPE
LDS = 1024                 # DH_FIT_LDS_POINTS: a model is staged up to it and streamed above
SMALL = dict(min_points=16, max_rms=np.inf)


@pytest.fixture(scope="module")
def ft():
    with fit.Fitter() as f:
        yield f


@contextlib.contextmanager
def gpu_set(v, t, B, st):
    """The set on the GPU in the state of the restated one."""
    with fit.ShapeBasis(B) as basis, fit.Subjects(v, t, basis, len(st)) as got:
        got.set_coeffs(st.state["coeffs"][:, :len(B)])
        for s in (0, len(st) - 1):
            pts, nrm = got.read(s)
            assert pts.tobytes() == st.pts[s].tobytes() and nrm.tobytes() == st.nrm[s].tobytes()
        yield got


@contextlib.contextmanager
def rig(Ks, V, u):
    with Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        yield views


def on_gpu(ft, got, views, frames, rec_in, sets=None, n_subjects=None, enrolled=None, frec=None, prm=None, device=False):
    """(subjects u32, records, poses, scores [m, n_subjects]) from the host form, or from the _device form on the current stream."""
    if not device:
        return ft.identify_subjects_views(frames, views, got, rec_in, sets=sets, n_subjects=n_subjects, enrolled=enrolled, fit_records=frec,
                                          params=prm, scores=True)
    import torch
    d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
    d = ft.identify_subjects_views(d_frames, views, got, to_device(rec_in), sets=None if sets is None else torch.from_numpy(np.asarray(sets, np.uint32).view(np.int32).copy()).cuda(),
                                   n_subjects=n_subjects, enrolled=None if enrolled is None else to_device(np.asarray(enrolled, np.uint8)),
                                   fit_records=None if frec is None else to_device(frec), params=prm, scores=True, device_out=True)
    torch.cuda.synchronize()
    ns = len(got) if n_subjects is None else n_subjects
    return (d[0].cpu().numpy().view(np.uint32), d[1].cpu().numpy().view(REC), d[2].cpu().numpy().view(INST),
            d[3].cpu().numpy().view(FREC).reshape(len(rec_in), ns))


def same(got, want, what):
    subjects, rec, poses, scores = got
    w_subjects, w_rec, w_poses, w_scores = want
    assert subjects.tobytes() == w_subjects.tobytes(), (what, subjects, w_subjects)
    assert rec.tobytes() == w_rec.tobytes(), (what, rec, w_rec)
    assert scores.tobytes() == w_scores.tobytes(), (what, scores, w_scores)
    assert poses.tobytes() == svs.as_records(w_poses).tobytes(), (what, poses, w_poses)


def both(ft, got, views, scene, inst, prm_kw, what, sets="own", n_subjects=None, enrolled=None, fit_status=None, device=False):
    """One identification on the GPU and in the restatement; everything equal.  scene: (frames, Ks, V, u, the restated set);
    sets: "own" -- the set each instance was built for --, None or a list.  Returns the restatement's answer."""
    frames, Ks, V, u, st = scene
    sets = ivs.sets_of(inst) if isinstance(sets, str) else sets
    frec = None
    if fit_status is not None:
        frec = np.zeros(len(inst), FREC)
        frec["status"] = fit_status
    out = on_gpu(ft, got, views, frames, svs.as_records(inst), sets, n_subjects, enrolled, frec, fit.ident_views_params(**prm_kw), device)
    ref = ivr.identify(frames, Ks, V, u, st, inst, sets, n_subjects, enrolled, fit_status, ivr.params(**prm_kw))
    same(out, ref, what)
    return ref


def opened(stack, g):
    """A gallery of ident_views_scenes on the GPU: (scene, instances, the set's handle, the view table)."""
    v, t, B, frames, Ks, V, u, inst, st = g
    return (frames, Ks, V, u, st), inst, stack.enter_context(gpu_set(v, t, B, st)), stack.enter_context(rig(Ks, V, u))


MESHES = [("255", 96, 96), ("256", 96, 96), ("257", 160, 120), ("strip%d" % (LDS - 1), 160, 120), ("strip%d" % LDS, 160, 120),
          ("strip%d" % (LDS + 1), 160, 120)]


@pytest.mark.parametrize("name,w,h", MESHES)
def test_every_mesh_size_staged_and_streamed(ft, name, w, h):
    """The lane stride of a pass, the strip below, at and above the LDS budget; three subjects, two heads seen by three cameras; the
    host form and, for every other case, the _device form."""
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery(name, 3, w, h, [0, 2]))
        ref = both(ft, got, views, scene, inst, SMALL, name, device=name in ("256", "strip%d" % LDS))
        assert (ref[1]["eligible"] >= 1).all() and (ref[1]["status"] == ir.OK).all(), ref[1]
        assert (ref[3]["steps"][ref[3]["status"] == fr.OK] > 0).all()


def test_every_mask_and_a_first_camera_that_is_not_0(ft):
    with contextlib.ExitStack() as stack:
        masks = [0b1, 0b11, 0b101, 0b111, 0b10, 0b110]
        scene, inst, got, views = opened(stack, ivs.gallery("162", 3, 96, 96, [0, 1, 2], sets=[0, 1, 2, 0, 1, 2], masks=masks, z=400.0))
        for device in (False, True):
            ref = both(ft, got, views, scene, inst, SMALL, "masks", device=device)
            assert ref[3]["views_used"][:, 0].tolist() == masks
        shifted = [dict(i, first_cam=1, views=m) for i, m in zip(inst, (0b1, 0b11, 0b10, 0b11, 0b1, 0b10))]
        for device in (False, True):
            ref = both(ft, got, views, scene, shifted, SMALL, "first_cam 1", device=device)
            assert ref[3]["views_used"][:, 0].tolist() == [0b1, 0b11, 0b10, 0b11, 0b1, 0b10] and (ref[1]["eligible"] >= 1).all()
        assert both(ft, got, views, scene, inst[:1], SMALL, "alone")[3].tobytes() != both(ft, got, views, scene, shifted[:1], SMALL, "shifted")[3].tobytes()


def test_a_mask_whose_bits_lie_at_and_above_bit_32_on_a_table_of_34_cameras(ft):
    """The mask crosses the lanes in two 32-bit halves: bits 32 and 33 alone, and bits 31 and 32 together."""
    with contextlib.ExitStack() as stack:
        masks = [(1 << 32) | (1 << 33), (1 << 31) | (1 << 32), 1 | (1 << 33)]
        scene, inst, got, views = opened(stack, ivs.gallery("162", 2, 48, 48, [1], sets=[0, 0, 0], masks=masks, n_cams=34, z=300.0))
        for device in (False, True):
            ref = both(ft, got, views, scene, inst, SMALL, "34 cameras", device=device)
            assert ref[3]["views_used"][:, 1].tolist() == masks and (ref[1]["eligible"] == 2).all() and (ref[1]["best"] == 1).all()
        past = [dict(inst[0], first_cam=1)]                                            # bit 33 from camera 1 on: camera 34 of 34
        assert both(ft, got, views, scene, past, SMALL, "camera 34", device=True)[1]["status"].tolist() == [ir.SKIPPED]


@pytest.mark.parametrize("n_subjects", [1, 2, 63, 64, 65])
def test_gallery_sizes_about_the_decide_waves_stride(ft, n_subjects):
    """S = 1 (no second), 2, one below, at and above the 64 lanes of the decide wave; every candidate eligible, so the best and
    the second come out of the whole reduction."""
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery("642", n_subjects, 96, 96, [n_subjects // 2]))
        ref = both(ft, got, views, scene, inst, SMALL, n_subjects, device=n_subjects in (2, 64))
        assert ref[1]["eligible"][0] == n_subjects and ref[1]["status"][0] == ir.OK
        assert (ref[1]["second"][0] == ir.UNKNOWN) == (n_subjects == 1)


def test_fewer_subjects_than_the_set_the_enrolment_mask_and_nobody_enrolled(ft):
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery("642", 5, 96, 96, [0, 4, 2], z=400.0))
        ref = both(ft, got, views, scene, inst, SMALL, "n_subjects 3 of 5", n_subjects=3)
        assert ref[3].shape == (3, 3) and ref[0].tolist()[0] == 0 and 4 not in ref[0].tolist()
        for device in (False, True):
            ref = both(ft, got, views, scene, inst, SMALL, "a mask", enrolled=[1, 0, 0, 1, 1], device=device)
            assert not ref[3][:, 1:3].tobytes().strip(b"\0") and (ref[1]["eligible"] == 3).all() and ref[0].tolist() == [0, 4, 3]
            ref = both(ft, got, views, scene, inst, SMALL, "nobody enrolled", enrolled=[0] * 5, device=device)
            assert (ref[1]["status"] == ir.NO_CANDIDATE).all() and not ref[3].tobytes().strip(b"\0")
            assert svs.as_records(ref[2]).tobytes() == svs.as_records(inst).tobytes()


@pytest.mark.parametrize("n_inst", [0, 1, 33])
def test_instance_counts(ft, n_inst):
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery("162", 2, 96, 96, [0, 1, 1], sets=[i % 3 for i in range(n_inst)], z=400.0))
        for device in (False, True):
            ref = both(ft, got, views, scene, inst, SMALL, n_inst, device=device)
            assert len(ref[0]) == n_inst and (ref[1]["status"] == ir.OK).all()
            assert ref[0].tolist() == [(0, 1, 1)[i % 3] for i in range(n_inst)]


@pytest.mark.parametrize("iterations", [0, 1, 4])
def test_iterations(ft, iterations):
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery("642", 3, 96, 96, [0, 1, 2, 1]))
        ref = both(ft, got, views, scene, inst, dict(SMALL, iterations=iterations), iterations, device=iterations in (0, 4))
        assert (ref[3]["steps"] <= iterations).all() and ref[3]["steps"].max() == iterations
        if iterations == 0:
            assert svs.as_records(ref[2]).tobytes() == svs.as_records(inst).tobytes()
        if iterations == 4:
            assert ref[0].tolist() == [0, 1, 2, 1]


def test_one_set_three_sets_with_instances_in_different_sets_and_no_sets_at_all(ft):
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery("162", 3, 96, 96, [1, 2, 0], sets=[2, 0, 1, 0, 2], z=400.0))
        for device in (False, True):
            ref = both(ft, got, views, scene, inst, SMALL, "three sets", device=device)
            assert ref[0].tolist() == [0, 1, 2, 1, 0]
            none = both(ft, got, views, scene, inst, SMALL, "sets NULL", sets=None, device=device)
            assert none[1][[1, 3]].tobytes() == ref[1][[1, 3]].tobytes() and none[3][[0, 2, 4]].tobytes() != ref[3][[0, 2, 4]].tobytes()
        one = (scene[0][:1],) + scene[1:]                                              # n_sets = 1: the instances of sets 1 and 2 are skipped
        ref = both(ft, got, views, one, inst, SMALL, "one set", device=True)
        assert ref[1]["status"].tolist() == [ir.SKIPPED, ir.OK, ir.SKIPPED, ir.OK, ir.SKIPPED]
        assert both(ft, got, views, one, inst, SMALL, "one set, sets NULL", sets=None)[3].tobytes() == none[3].tobytes()


def test_a_pair_that_ends_few_points_and_one_that_ends_singular_among_eligible_ones(ft):
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery("642", 3, 96, 96, [0, 1, 2, 1], z=400.0))
        free = ivr.identify(*scene[:5], inst, ivs.sets_of(inst), prm=ivr.params(**SMALL))[3]["points"]
        limit = int(np.sort(free.reshape(-1))[len(inst)])                               # above the fewest pairs' points, below most
        ref = both(ft, got, views, scene, inst, dict(min_points=limit, max_rms=np.inf), "few points", device=True)
        assert sorted(set(ref[3]["status"].reshape(-1).tolist())) == [fr.OK, fr.FEW_POINTS] and ref[0].tolist() == [0, 1, 2, 1]
        assert ((ref[1]["eligible"] >= 1) & (ref[1]["eligible"] <= 3)).all() and (ref[1]["eligible"] < 3).any()
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.flat_twin())
        for device in (False, True):
            ref = both(ft, got, views, scene, inst, dict(SMALL, lam=0.0, iterations=3), "singular", device=device)
            assert ref[3]["status"][0].tolist() == [fr.SINGULAR, fr.OK] and ref[1][0]["best"] == 1 and ref[1][0]["eligible"] == 1


def test_two_identical_candidates_under_both_ratios(ft):
    g = ivs.gallery("642", 3, 96, 96, [1, 1])
    g[8].set_coeffs(np.array([[0.1], [0.1], [-0.4]]))
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, g)
        for ratio, status in ((1.0, ir.OK), (1.5, ir.AMBIGUOUS)):
            ref = both(ft, got, views, scene, inst, dict(SMALL, min_ratio=ratio), ratio, device=ratio > 1)
            assert (ref[1]["status"] == status).all() and (ref[1]["best"] == 0).all() and (ref[1]["second"] == 1).all()
            assert (ref[0] == (0 if status == ir.OK else ir.UNKNOWN)).all()


def test_a_view_with_no_pixel_and_the_instances_the_device_skips_and_the_host_form_refuses(ft):
    """A blank view takes part and is missing from views_used.  What the host form refuses per instance, the device skips as a
    whole: no view, a camera >= n, a set >= n_sets, a NaN in t, an R outside the tolerance (one inside it takes part), a scale that
    carries the set's bound past the extent; a fit record that is not OK is skipped by both forms."""
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery("642", 3, 96, 96, [0, 1, 2], sets=[0, 1, 2, 0, 1, 2, 0, 1], blank=((1, 2),)))
        frames = scene[0]
        for device in (False, True):
            ref = both(ft, got, views, scene, inst, SMALL, "a blank view", device=device)
            assert (ref[3]["views_used"][[1, 4, 7]] == 0b011).all() and (ref[3]["views_used"][[0, 2, 3, 5, 6]] == 0b111).all()
            assert (ref[1]["status"] == ir.OK).all()
        status = np.zeros(len(inst), np.uint32)
        status[[2, 5]] = (fr.FEW_POINTS, fr.SINGULAR)
        for device in (False, True):
            ref = both(ft, got, views, scene, inst, SMALL, "fit records", fit_status=status, device=device)
            assert ref[1]["status"][[2, 5]].tolist() == [ir.SKIPPED] * 2 and not ref[3][[2, 5]].tobytes().strip(b"\0")
        bad = [dict(i) for i in inst]
        bad[0]["views"] = 0
        bad[1]["views"] = 0b1000
        bad[2]["set"] = 3
        bad[3]["t"] = np.array([np.nan, 0.0, 0.0], np.float32)
        bad[4]["R"] = (inst[4]["R"] * np.float32(1.02)).astype(np.float32)            # R R^T = 1.0404 I: outside the tolerance of 0.02
        bad[5]["R"] = (inst[5]["R"] * np.float32(1.005)).astype(np.float32)           # 1.010025 I: within it, takes part
        bad[6]["scale"] = np.float32(40.0)                                             # 40 * the bound (about 150 mm) > 4096
        ref = both(ft, got, views, scene, bad, SMALL, "faulty instances", device=True)
        assert ref[1]["status"].tolist() == [ir.SKIPPED] * 5 + [ir.OK, ir.SKIPPED, ir.OK], ref[1]
        for i in (0, 1, 2, 3, 4, 6):                                                    # skipped: the input copied through, bit for bit
            assert ref[0][i] == ir.UNKNOWN and svs.as_records(ref[2][i:i + 1]).tobytes() == svs.as_records(bad[i:i + 1]).tobytes()
        for host_bad, text in ((0, "seen by no view"), (1, "names camera 3 of 3"), (2, "names set 3 of 3"), (3, "non-finite"), (4, "instance 4"), (6, "spans")):
            only = [dict(i) for i in inst]
            only[host_bad] = bad[host_bad]
            with pytest.raises(_lib.DepthheadError, match=text):
                ft.identify_subjects_views(frames, views, got, svs.as_records(only), sets=ivs.sets_of(only))
            skip = np.zeros(len(inst), FREC)                                           # ... a fit record that is not OK comes after the
            skip["status"][host_bad] = fr.FEW_POINTS                                    # view, the camera and the set, before R, t and scale
            if host_bad < 3:
                with pytest.raises(_lib.DepthheadError, match=text):
                    ft.identify_subjects_views(frames, views, got, svs.as_records(only), sets=ivs.sets_of(only), fit_records=skip)
            else:
                rec = ft.identify_subjects_views(frames, views, got, svs.as_records(only), sets=ivs.sets_of(only), fit_records=skip)[1]
                assert rec["status"][host_bad] == ir.SKIPPED


@pytest.mark.parametrize("points,part", [(16384, True), (16385, False)])
def test_two_views_of_a_strip_at_the_term_limit_and_one_point_above(ft, points, part):
    """popcount(views) * points at exactly DH_FIT_MAX_POINTS = 32768 takes part; one point more and the device skips the instance
    and the host form refuses it; with one view the longer strip takes part."""
    with contextlib.ExitStack() as stack:
        scene, inst, got, views = opened(stack, ivs.gallery("fine%d" % points, 2, 160, 120, [1], sets=[0, 0], masks=[0b101, 0b100]))
        ref = both(ft, got, views, scene, inst, SMALL, points, device=True)
        assert ref[1]["status"].tolist() == [ir.OK if part else ir.SKIPPED, ir.OK] and (ref[3]["views_used"][1] == 0b100).all()
        if part:
            both(ft, got, views, scene, inst, SMALL, "host form")
        else:
            with pytest.raises(_lib.DepthheadError, match="instance 0 sums 32770 terms"):
                ft.identify_subjects_views(scene[0], views, got, svs.as_records(inst))


def test_the_one_view_identity_against_the_single_view_call_with_cameras(ft):
    """One view, V = I, u = 0, n_sets = 1: every subject, record byte and refitted pose equals dh_fit_identify_subjects_cameras on
    the same pose, and every score equals the single-view score in its first 24 bytes -- on the GPU, call against call."""
    v, t, B, frames, K, inst, frames4, Ks, V, u, world, st = ivs.single_view_twin("642", 3, 96, 96, [0, 1, 2, 1])
    with gpu_set(v, t, B, st) as got, Cameras(Ks) as cams, fit.Views(cams, V, u) as views:
        for prm_kw in (SMALL, dict(SMALL, iterations=0), dict(min_points=16, max_rms=1.0)):
            for device in (False, True):
                multi = on_gpu(ft, got, views, frames4, svs.as_records(world), prm=fit.ident_views_params(**prm_kw), device=device)
                single = ft.identify_subjects(frames, got, ss.as_records(inst), cams, params=fit.ident_params(**prm_kw), scores=True)
                assert multi[0].tobytes() == single[0].tobytes() and multi[1].tobytes() == single[1].tobytes(), (multi[1], single[1])
                for name in SCORE1.names:
                    assert (multi[3][name] == single[3][name]).all(), name
                assert (multi[3]["views_used"] == 1).all()
                for name in ("R", "t", "scale"):
                    assert multi[2][name].tobytes() == single[2][name].tobytes(), name
                assert multi[2]["first_cam"].tolist() == single[2]["frame"].tolist() and (multi[2]["views"] == 1).all()
        same(multi, ivr.identify(frames4, Ks, V, u, st, world, prm=ivr.params(**prm_kw)), "the restatement")


def test_host_form_against_the_device_form_after_a_device_fit_between_guard_bands_and_two_runs(ft):
    """The _device form on a side stream, fed by a device multi-view fit's instances and records, every output written between
    guard bands; the host form from the same fit read back; a second run of each: all equal the restatement.  One moment of the
    rig: five starts of one head under different masks, the last of which sees only a camera whose frame is empty."""
    import torch
    masks = [0b111, 0b011, 0b110, 0b101, 0b100]
    v, t, B, frames, Ks, V, u, inst, st = ivs.gallery("642", 3, 96, 96, [1], sets=[0] * 5, masks=masks, nudge=(4.0, -3.0, 5.0), blank=((0, 2),))
    lib = _lib.load()
    with gpu_set(v, t, B, st) as got, rig(Ks, V, u) as views, fit.Model(st.pts[0], st.nrm[0]) as generic:
        m, ns = len(inst), 3
        stream = torch.cuda.Stream()
        band = 256
        sizes = {"sub": 4 * m, "rec": REC.itemsize * m, "poses": INST.itemsize * m, "scores": FREC.itemsize * m * ns}
        d_frames = torch.from_numpy(frames.view(np.int16).copy()).cuda()
        runs = []
        for _ in range(2):
            out = {k: torch.full((2 * band + n,), 0xCD, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                d_inst, d_frec = ft.fit_views(d_frames[0], [generic], svs.as_records(inst), views, device_out=True, stream=stream.cuda_stream)
                fit.check(lib.dh_fit_identify_subjects_views_device(
                    ft._h, C.c_void_p(d_frames.data_ptr()), C.c_uint32(1), 96, 96, views._h, got._h, C.c_void_p(d_inst.data_ptr()), C.c_uint32(m), None, None,
                    C.c_uint32(ns), C.c_void_p(d_frec.data_ptr()), C.byref(fit.ident_views_params(**SMALL)), C.c_void_p(out["sub"].data_ptr() + band),
                    C.c_void_p(out["rec"].data_ptr() + band), C.c_void_p(out["poses"].data_ptr() + band), C.c_void_p(out["scores"].data_ptr() + band),
                    C.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            raw = {k: o.cpu().numpy() for k, o in out.items()}
            for k, r in raw.items():
                assert (r[:band] == 0xCD).all() and (r[-band:] == 0xCD).all(), k
            fitted, frec = d_inst.cpu().numpy().view(INST), d_frec.cpu().numpy().view(FREC)
            runs.append((fitted.tobytes(), frec.tobytes()) + tuple(raw[k][band:-band].tobytes() for k in sizes))
        assert runs[0] == runs[1]
        assert frec["status"].tolist() == [fr.OK] * 4 + [fr.FEW_POINTS] and frec["views_used"].tolist() == [0b011, 0b011, 0b010, 0b001, 0]
        ref_inst = [ivs.instance(r["R"], r["t"], int(r["views"]), int(r["first_cam"]), r["scale"]) for r in fitted]
        ref = ivr.identify(frames, Ks, V, u, st, ref_inst, None, None, None, frec["status"], ivr.params(**SMALL))
        dev = (raw["sub"][band:-band].view(np.uint32), raw["rec"][band:-band].view(REC), raw["poses"][band:-band].view(INST),
               raw["scores"][band:-band].view(FREC).reshape(m, ns))
        same(dev, ref, "device form")
        assert ref[1]["status"].tolist() == [ir.OK] * 4 + [ir.SKIPPED] and ref[0].tolist() == [1, 1, 1, 1, ir.UNKNOWN]
        for _ in range(2):
            same(ft.identify_subjects_views(frames, views, got, fitted, fit_records=frec, params=fit.ident_views_params(**SMALL), scores=True), ref, "host form")


def test_no_poses_and_no_scores(ft):
    """poses_out NULL and scores NULL, in both forms: the subjects and the records are what they are with them."""
    import torch
    v, t, B, frames, Ks, V, u, inst, st = ivs.gallery("642", 3, 96, 96, [2, 0])
    lib, vp = _lib.load(), _lib.vp
    sets = np.arange(2, dtype=np.uint32)
    ref = ivr.identify(frames, Ks, V, u, st, inst, sets, prm=ivr.params(**SMALL))
    rin, prm = svs.as_records(inst), fit.ident_views_params(**SMALL)
    with gpu_set(v, t, B, st) as got, rig(Ks, V, u) as views:
        sub, rec = np.zeros(2, np.uint32), np.zeros(2, REC)
        fit.check(lib.dh_fit_identify_subjects_views(ft._h, vp(frames), C.c_uint32(2), 96, 96, views._h, got._h, vp(rin), C.c_uint32(2), vp(sets), None,
                                                     C.c_uint32(3), None, C.byref(prm), vp(sub), vp(rec), None, None))
        assert sub.tobytes() == ref[0].tobytes() and rec.tobytes() == ref[1].tobytes()
        d_frames, d_in, d_sets = torch.from_numpy(frames.view(np.int16).copy()).cuda(), to_device(rin), to_device(sets)
        d_sub, d_rec = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2 * REC.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fit.check(lib.dh_fit_identify_subjects_views_device(ft._h, C.c_void_p(d_frames.data_ptr()), C.c_uint32(2), 96, 96, views._h, got._h,
                                                            C.c_void_p(d_in.data_ptr()), C.c_uint32(2), C.c_void_p(d_sets.data_ptr()), None, C.c_uint32(3),
                                                            None, C.byref(prm), C.c_void_p(d_sub.data_ptr()), C.c_void_p(d_rec.data_ptr()), None, None, None))
        torch.cuda.synchronize()
        assert d_sub.cpu().numpy().tobytes() == ref[0].tobytes() and d_rec.cpu().numpy().tobytes() == ref[1].tobytes()


def test_recognise_subjects_views_against_the_restated_driver_on_the_evaluations_probes(ft):
    """fit.recognise_subjects_views over the 16 probes of the evaluation -- 12 of enrolled subjects, 4 of a stranger, each one
    moment of its own rig -- with the shipped defaults: the bytes of tests/ident_views_ref.py, and with them 12 right answers and 4
    times DH_IDENT_FAR."""
    st, enrolled, rigs, probes, starts, truth = ivs.evaluation()
    want_sub, want_rec, want_poses, want_frec = ivs.evaluation_result()
    v, t, n, B = ss.generic()
    per = len(probes) // len(rigs)
    with gpu_set(v, t, B, st) as got, fit.Model(v, n) as generic:
        for r, (Ks, V, u) in enumerate(rigs):
            with rig(Ks, V, u) as views:
                for i in range(r * per, (r + 1) * per):
                    subjects, rec, poses, frec = fit.recognise_subjects_views(ft, probes[i], views, got, svs.as_records(starts[i:i + 1]), generic, enrolled=enrolled)
                    assert subjects.tobytes() == want_sub[i:i + 1].tobytes() and rec.tobytes() == want_rec[i:i + 1].tobytes(), (i, rec, want_rec[i])
                    assert poses.tobytes() == svs.as_records(want_poses[i:i + 1]).tobytes()
                    w = want_frec[i]
                    assert (int(frec["status"][0]), int(frec["points"][0]), int(frec["sum_r2_fixed"][0]), int(frec["views_used"][0])) == \
                        (w["status"], w["points"], w["sum_r2_fixed"], w["views_used"])
                empty = fit.recognise_subjects_views(ft, probes[r * per], views, got, svs.as_records([]), generic, enrolled=enrolled)
                assert [len(x) for x in empty] == [0, 0, 0, 0]
    assert want_sub.tolist() == [ir.UNKNOWN if who is None else who for who in truth]
    assert want_rec["status"].tolist() == [ir.FAR if who is None else ir.OK for who in truth]
