"""Galleries and scenes shared by the multi-view identification tests (test_ident_views_ref.py on the CPU,
test_gpu_ident_views.py on the GPU).  The galleries are ident_scenes' -- any mesh, any size, subjects that
differ by one coefficient -- seen by the cameras of an arc (view_fit_scenes.arc): every SET holds one subject's own model at a
seeded world pose, splatted into each camera's frame at the composite camera pose (cheap at any size).  The evaluation is
shape_views_scenes' rig of three 160x120 cameras: three subjects enrolled from the middle camera's frames of four sets each,
four further sets of each and of a stranger as probes.  What is expensive is computed once."""
import functools

import numpy as np

import ident_scenes as isc
import ident_views_ref as ivr
import shape_scenes as ss
import shape_views_scenes as svs
import subjects_ref as sb
import surface_ref as su
import surface_scenes as us
import view_fit_scenes as vs
from depthhead_amd import fit, render, synth


def spread(n_cams, half=35.0):
    """The yaws of n_cams cameras on the arc, -half .. +half degrees (one camera: 0)."""
    return tuple(np.linspace(-half, half, n_cams)) if n_cams > 1 else (0.0,)


def world_pose(seed, max_deg=10.0, reach=25.0):
    """A seeded world pose near the origin the cameras look at: (R [3, 3] f32, t [3] f32)."""
    u = synth.SplitMix(330000 + seed).uniform(6)
    return render.euler_to_matrix((2.0 * u[:3] - 1.0) * max_deg).astype(np.float32), (reach * (2.0 * u[3:] - 1.0)).astype(np.float32)


def instance(R, t, views=0b111, first_cam=0, scale=1.0, set_=0):
    return {"first_cam": int(first_cam), "views": int(views), "R": np.asarray(R, np.float32).reshape(3, 3), "t": np.asarray(t, np.float32).reshape(3),
            "scale": np.float32(scale), "set": int(set_)}


def sets_of(instances):
    """The `sets` argument of a call over `instances`: the set each was built for."""
    return [i["set"] for i in instances]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """ident_scenes.mesh, and "fine<n>": a strip of n vertices 0.0125 mm apart (16384 of them are 205 mm long, so the field stays
    inside DH_SHAPE_MAX_FIELD), with ident_scenes' field."""
    if not name.startswith("fine"):
        return isc.mesh(name)
    v, t = us.strip_mesh(int(name[4:]), step=0.0125)
    return v, t, (0.5 * (v * np.array([1.0, -0.5, 0.0], np.float32))[None] + 0.1 * isc.sc.seeded_fields(v, 1, 40 + len(v))).astype(np.float32)


def gallery(name, n_subjects, w, h, truth, masks=None, sets=None, n_cams=3, first_cam=0, seed=5, surface=False, nudge=(1.5, -1.0, 2.0),
            z=800.0, blank=()):
    """(v, t, B, frames [len(truth), n_cams, h, w], Ks [n_cams, 3, 3], V, u, instances, the restated set).  Set s shows subject
    truth[s]'s own model at a seeded world pose through every camera, except the (set, camera) pairs of `blank`, which stay empty.
    Instance i belongs to set sets[i] (default: one instance per set, i), carries masks[i] (default: all cameras from first_cam
    on) and is that set's pose moved by `nudge` mm, so a refit has something to do; sets_of(instances) is the call's `sets`."""
    v, t, B = mesh(name)
    st = su.Set(v, t, B, n_subjects, max_offset=16.0) if surface else sb.Set(v, t, B, n_subjects)
    st.set_coeffs(isc.coefficients(n_subjects))
    if surface:
        for s in range(n_subjects):
            st.set_offsets(s, us.bump(v, (7 * s + 3) % len(v), 5.0 - 2.0 * (s % 3), 0.2 * float(np.ptp(v, axis=0).max())))
    V, u = fit.views_from_rig(*vs.arc(spread(n_cams), [z] * n_cams))
    K = synth.default_intrinsic(w, h)
    Ks = np.ascontiguousarray(np.broadcast_to(K, (n_cams, 3, 3)))
    n_sets = max(len(truth), 1)
    frames = np.zeros((n_sets, n_cams, h, w), np.uint16)
    poses = []
    for s, who in enumerate(truth):
        R, p = world_pose(seed * 100 + s)
        poses.append((R, p))
        for c in range(n_cams):
            if (s, c) in blank:
                continue
            Rc, tc = vs.camera_pose(V[c], u[c], R, p)
            frames[s, c] = us.splat(st.pts[who], K, us.instance(0, Rc, tc), w, h, seed=(seed * 100 + s) * 64 + c)
    sets = list(range(len(truth))) if sets is None else list(sets)
    full = (1 << (n_cams - first_cam)) - 1
    inst = []
    for i, s in enumerate(sets):
        R, p = poses[s % len(poses)] if poses else world_pose(seed * 100)
        inst.append(instance(R, p + np.asarray(nudge, np.float32), full if masks is None else masks[i], first_cam, set_=s))
    return v, t, B, frames, Ks, V, u, inst, st


def single_view_twin(name, n_subjects, w, h, truth, **kw):
    """ident_scenes.gallery as a rig whose cameras all stand at the world's origin (V = I, u = 0): (v, t, B, frames [n, h, w], K, the
    single-view instances, frames [1, n, h, w], Ks, V, u, the world instances -- instance f sees camera f alone --, the set)."""
    v, t, B, frames, K, inst, st = isc.gallery(name, n_subjects, w, h, truth, **kw)
    n = len(frames)
    Ks = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float32), (n, 3, 3)))
    V, u = np.ascontiguousarray(np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3))), np.zeros((n, 3), np.float32)
    world = [instance(i["R"], i["t"], 0b1, i["frame"], i["scale"]) for i in inst]
    return v, t, B, frames, K, inst, frames[None], Ks, V, u, world, st


def flat_twin():
    """ident_scenes.flat_gallery seen by two cameras that both stand at the world's origin (V = I, u = 0) before the same wall:
    (v, t, B, frames [1, 2, h, w], Ks, V, u, one world instance with both views, the set of 2).  With lambda = 0 the plane's refit
    ends DH_FIT_SINGULAR -- its sums are the single view's, twice -- and the curved subject fits."""
    v, t, B, frames, K, inst, st = isc.flat_gallery()
    Ks = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float32), (2, 3, 3)))
    V, u = np.ascontiguousarray(np.broadcast_to(np.eye(3, dtype=np.float32), (2, 3, 3))), np.zeros((2, 3), np.float32)
    return v, t, B, np.stack([frames[0], frames[0]])[None], Ks, V, u, [instance(inst[0]["R"], inst[0]["t"], 0b11)], st


# ---- the evaluation: shape_views_scenes' subjects, eight sets each
EVAL_COEFFS = ((0.08, -0.07, 0.06, 0.0), (-0.06, 0.05, 0.04, 0.0), (0.03, 0.08, -0.07, 0.0))
EVAL_STRANGER = (-0.07, -0.06, 0.09, 0.0)
EVAL_SEED, EVAL_ENROL, EVAL_SETS = 20, 4, 8
ALL, MIDDLE = 0b111, 1 << svs.MIDDLE


@functools.lru_cache(maxsize=None)
def evaluation():
    """(the enrolled set of 4 -- subjects 0 .. 2 adapted by subjects_ref.adapt_subjects over the middle camera's frames of sets
    0 .. 3, subject 3 left the generic head --, enrolled [4], rigs: (Ks, V, u) of each of the four people's scenes (a scene's
    camera distances are its own), probe frames [16, 3, h, w], probe starts (world, all three views), truth [16]: the subject of
    each probe, None for the stranger's; probe i was taken by rig i // 4)."""
    v, t, _, B = ss.generic()
    st = sb.Set(v, t, B, 4)
    frames, starts, who, probes, p_starts, truth, rigs = [], [], [], [], [], [], []
    Ks = None
    for s, c in enumerate(EVAL_COEFFS + (EVAL_STRANGER,)):
        f, Ks, V, u, pos, Rs = svs.subject(EVAL_SEED + s, n_sets=EVAL_SETS, c_true=c)
        rigs.append((Ks, V, u))
        rough = svs.rough_instances(EVAL_SEED + s, pos, Rs)
        if s < len(EVAL_COEFFS):
            for it in svs.single_view(rough[:EVAL_ENROL], V, u):
                starts.append(dict(it, frame=len(frames)))
                frames.append(f[it["frame"], svs.MIDDLE])
                who.append(s)
        for i in range(EVAL_ENROL, EVAL_SETS):
            p_starts.append(dict(rough[i]))
            probes.append(f[i])
            truth.append(s if s < len(EVAL_COEFFS) else None)
    sb.adapt_subjects(np.stack(frames), Ks[svs.MIDDLE], st, starts, who, rounds=6)
    return st, np.array([1, 1, 1, 0], np.uint8), rigs, np.stack(probes), p_starts, truth


@functools.lru_cache(maxsize=None)
def evaluation_result(views=ALL, max_rms=ivr.DEFAULT_MAX_RMS, min_points=64):
    """ident_views_ref.recognise_subjects_views over each probe with the generic head for the first fit: (subjects u32 [16],
    records [16], poses, the generic fit's records)."""
    st, enrolled, rigs, probes, starts, _ = evaluation()
    v, _, n, _ = ss.generic()
    subjects, records, poses, recs = [], [], [], []
    for i, (frames, start) in enumerate(zip(probes, starts)):
        Ks, V, u = rigs[i // (EVAL_SETS - EVAL_ENROL)]
        s, r, p, fr_ = ivr.recognise_subjects_views(frames, Ks, V, u, st, [dict(start, views=views)], (v, n), enrolled, None,
                                                    ivr.params(max_rms=max_rms, min_points=min_points))
        subjects.append(s[0]); records.append(r[0]); poses.append(p[0]); recs.append(fr_[0])
    return np.array(subjects, np.uint32), np.array(records, ivr.RECORD_DTYPE), poses, recs
