"""Galleries and scenes shared by the identification tests (test_ident_ref.py on the CPU, test_gpu_ident.py on the GPU; DESIGN.md
section 27): small galleries of any mesh and any size whose subjects differ by one coefficient, with frames splatted from a
subject's own model (cheap at any size), and the evaluation -- three subjects of section 26's kind enrolled from eight frames
each, four held-out frames of each and of a stranger as probes.  What is expensive is computed once."""
import functools

import numpy as np

import ident_ref as ir
import subjects_ref as sb
import subjects_scenes as sc
import surface_ref as su
import surface_scenes as us
from depthhead_amd import synth


@functools.lru_cache(maxsize=None)
def mesh(name):
    """name -> (verts, tris, one field): 4, 162, 642, 255, 256, 257 and 2562 vertices, and strips of any size.  The field is a
    stretch along x with a squeeze along y, 0.5 and 0.25 of the vertex -- smooth, and no pose can absorb it, so a splatted frame
    tells subjects apart -- plus a seeded +-2 mm a component."""
    if name.startswith("strip"):
        v, t = us.strip_mesh(int(name[5:]))
    else:
        tetra = (np.array([(0, 0, 0), (40, 0, 0), (0, 40, 0), (0, 0, 40)], np.float32), np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.uint32))
        v, t = {"4": lambda: tetra, "162": lambda: synth.head_mesh(2), "642": lambda: synth.head_mesh(3), "255": lambda: sc.lathe_mesh(11, 23), "256": lambda: sc.lathe_mesh(2, 127),
                "257": lambda: sc.lathe_mesh(15, 17), "2562": lambda: synth.head_mesh(4)}[name]()
    return v, t, (0.5 * (v * np.array([1.0, -0.5, 0.0], np.float32))[None] + 0.1 * sc.seeded_fields(v, 1, 40 + len(v))).astype(np.float32)


def coefficients(n_subjects):
    """Subject s's one coefficient: spread over +-0.4 (max_coeff is 0.5), none equal to another."""
    return np.linspace(-0.4, 0.4, n_subjects).reshape(-1, 1) if n_subjects > 1 else np.array([[0.25]])


def gallery(name, n_subjects, w, h, truth, seed=5, surface=False, nudge=(1.5, -1.0, 2.0), z=800.0):
    """(v, t, B, frames [len(truth), h, w], K, instances, the restated set): frame f shows subject truth[f]'s own model at a seeded
    pose (splatted), and instance f is that pose moved by `nudge` mm, so a refit has something to do.  A surface set also
    carries a seeded bump per subject."""
    v, t, B = mesh(name)
    st = su.Set(v, t, B, n_subjects, max_offset=16.0) if surface else sb.Set(v, t, B, n_subjects)
    st.set_coeffs(coefficients(n_subjects))
    if surface:
        for s in range(n_subjects):
            st.set_offsets(s, us.bump(v, (7 * s + 3) % len(v), 5.0 - 2.0 * (s % 3), 0.2 * float(np.ptp(v, axis=0).max())))
    K = synth.default_intrinsic(w, h)
    frames, inst = [], []
    for f, s in enumerate(truth):
        true = us.instance(f, *us.pose(seed * 100 + f, w, h, z=z))
        frames.append(us.splat(st.pts[s], K, true, w, h, seed=seed * 100 + f))
        inst.append(dict(true, t=true["t"] + np.asarray(nudge, np.float32)))
    return v, t, B, np.stack(frames) if frames else np.zeros((1, h, w), np.uint16), K, inst, st


def flat_gallery(w=160, h=120, n=9, step=20.0):
    """(v, t, B, frames [1, h, w], K, instances, the restated set of 2): a flat grid of n x n vertices facing the camera whose one
    field is a bowl along z.  Subject 0, at coefficient 0, is the plane of tests/test_fit_ref.py -- turned a little before a wall
    with lambda = 0 its refit ends DH_FIT_SINGULAR --, subject 1 is curved and fits."""
    g = (np.arange(n) - (n - 1) / 2.0) * step
    x, y = np.meshgrid(g, g)
    v = np.stack([x.ravel(), y.ravel(), np.zeros(n * n)], axis=1).astype(np.float32)
    q = np.array([(r * n + c, r * n + c + 1, (r + 1) * n + c, (r + 1) * n + c + 1) for r in range(n - 1) for c in range(n - 1)])
    t = np.concatenate([q[:, [0, 2, 1]], q[:, [1, 2, 3]]]).astype(np.uint32)       # wound so that the normals are (0, 0, -1)
    B = np.zeros((1, n * n, 3), np.float32)
    B[0, :, 2] = 0.002 * (v[:, 0] ** 2 + v[:, 1] ** 2)
    st = sb.Set(v, t, B, 2)
    st.set_coeffs(np.array([[0.0], [0.4]]))
    assert (st.nrm[0] == np.array([0, 0, -1], np.float32)).all()
    K = synth.default_intrinsic(w, h)
    from depthhead_amd import render
    inst = [us.instance(0, render.euler_to_matrix((0, 4, 3)), (0.0, 0.0, 810.0))]
    return v, t, B, np.full((1, h, w), 800, np.uint16), K, inst, st


# ---- the evaluation: surface_scenes' subjects, twelve poses each
EVAL_SEEDS, EVAL_STRANGER, EVAL_ENROL, EVAL_POSES = (12, 13, 14), 15, 8, 12


@functools.lru_cache(maxsize=None)
def evaluation():
    """(the enrolled set of 4 -- subjects 0 .. 2 refined from frames 0 .. 7 of seeds 12 .. 14, subject 3 left the generic head --,
    enrolled [4], K, probe frames [16, h, w], probe starts, truth [16]: the subject of each probe, None for the stranger's)."""
    v, t, _, B = us.eval_generic()
    st = su.Set(v, t, B, 4, max_offset=16.0)
    frames, starts, who, probes, p_starts, truth = [], [], [], [], [], []
    K = None
    for s, seed in enumerate(EVAL_SEEDS + (EVAL_STRANGER,)):
        f, K, pos, Rs = us.eval_subject(seed, poses=EVAL_POSES)
        rough = us.eval_starts(seed, pos, Rs)
        if seed != EVAL_STRANGER:
            for i in range(EVAL_ENROL):
                starts.append(dict(rough[i], frame=len(frames)))
                frames.append(f[i])
                who.append(s)
        for i in range(EVAL_ENROL, EVAL_POSES):
            p_starts.append(dict(rough[i], frame=len(probes)))
            probes.append(f[i])
            truth.append(s if seed != EVAL_STRANGER else None)
    su.refine_subjects(np.stack(frames), K, st, starts, who, rounds=6)
    return st, np.array([1, 1, 1, 0], np.uint8), K, np.stack(probes), p_starts, truth


@functools.lru_cache(maxsize=None)
def evaluation_result(max_rms=ir.DEFAULT_MAX_RMS):
    """ident_ref.recognise_subjects over the probes with the shipped defaults (the generic head for the first fit)."""
    st, enrolled, K, probes, starts, _ = evaluation()
    v, _, n, _ = us.eval_generic()
    return ir.recognise_subjects(probes, K, st, starts, (v, n), enrolled, None, ir.params(max_rms=max_rms))
