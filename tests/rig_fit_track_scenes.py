"""Sequences shared by the rig fit tracker's tests (test_rig_fit_track_ref.py on the CPU, test_gpu_rig_fit_tracker.py on the GPU):
the head of tests/view_fit_scenes.py (head_mesh(2) at a seeded world pose, its torso box, three cameras on an arc) moving
STEP_MM in a seeded direction and STEP_YAW degrees about the world's y axis per step, rendered by the renderer's restatement
with the sensor model, and what a rig tracker step would report of it made by hand: one dh_rig_person whose world is the truth
plus a 60 mm offset, and in its best camera one dh_head whose angles are the truth's in that camera's frame on the forest's
3-degree grid.  No forest is needed.  Every sequence is computed once and handed out read-only."""
import functools

import numpy as np

import fit_scenes as fs
import render_ref as rr
import view_fit_scenes as vs
from depthhead_amd import _lib, fit, render, synth

STEP_MM, STEP_YAW = 5.0, 2.0
BIN = 3.14159 / 60.0
MAX_HEADS = 2
PERSONS, SLOTS = _lib.RIG_MAX_PERSONS, _lib.RIG_MAX_TRACKS


def person(pos, R, V, u, first, views, best, pid, seed, offset_mm=60.0, head=0):
    """(dh_rig_person, dh_head) as a rig step would report the head at world (pos, R) seen by the cameras first + k of the set
    bits k of `views`: world `offset_mm` off in a seeded direction and rounded to integers, best_cam = first + best, and that
    camera's head with the angles of V[best_cam] R rounded to multiples of 3.14159 / 60."""
    d = 2.0 * synth.SplitMix(730000 + seed).uniform(3) - 1.0
    d = d / np.sqrt((d * d).sum())
    p = np.zeros((), _lib.RIG_PERSON_DTYPE)
    world = np.round(np.asarray(pos, np.float64) + offset_mm * d)
    b = first + best
    p["views"], p["mass"], p["cell"], p["n_views"], p["world"] = views, 100 * bin(views).count("1"), world, bin(views).count("1"), world
    p["id"], p["best_cam"], p["best_head"] = pid, b, head
    Vb, ub = np.asarray(V[b], np.float64), np.asarray(u[b], np.float64)
    hd = np.zeros((), _lib.HEAD_DTYPE)
    hd["pose"]["mid_point"] = np.round(Vb @ world + ub)
    hd["pose"]["rotation"] = np.round(np.radians(fit.matrix_to_euler(Vb @ np.asarray(R, np.float64))) / BIN) * BIN
    hd["support"]["windows"], hd["support"]["mass"], hd["support"]["total_mass"] = 10, 100, 1000
    return p, hd


def rig_inputs(n_cams, n_rigs, items, max_heads=MAX_HEADS):
    """(n_heads [n_cams], heads [n_cams, max_heads], n_persons [n_rigs], persons [n_rigs, 16]) from (rig, person, head) items in
    the order of their person index."""
    n_heads, heads = np.zeros(n_cams, np.uint32), np.zeros((n_cams, max_heads), _lib.HEAD_DTYPE)
    n_persons, persons = np.zeros(n_rigs, np.uint32), np.zeros((n_rigs, PERSONS), _lib.RIG_PERSON_DTYPE)
    for g, p, hd in items:
        persons[g, n_persons[g]] = p
        n_persons[g] += 1
        b, j = int(p["best_cam"]), int(p["best_head"])
        heads[b, j] = hd
        n_heads[b] = max(n_heads[b], j + 1)
    return n_heads, heads, n_persons, persons


@functools.lru_cache(maxsize=None)
def sequence(seed, steps=8, w=160, h=120, gone=(), lead=0):
    """(frames [steps, lead + 3, h, w] u16, Ks, V, u of the lead + 3 cameras, true positions [steps, 3] f64, true R [steps, 3, 3]
    f64).  The three cameras of the arc are cameras lead .. lead + 2; the `lead` cameras before them stand where camera 0 of
    the arc stands and see an empty frame (a rig of their own).  The steps listed in `gone` are empty in every camera."""
    pos0, R0, dists = vs.truth(seed)
    Ra, ta = vs.arc(vs.YAWS[3], dists)
    Ra, ta = np.concatenate([Ra[:1]] * lead + [Ra]), np.concatenate([ta[:1]] * lead + [ta])
    V, u = fit.views_from_rig(Ra, ta)
    n = lead + 3
    K = synth.default_intrinsic(w, h)
    Ks = np.ascontiguousarray(np.broadcast_to(K, (n, 3, 3)))
    un = synth.SplitMix(740000 + seed).uniform(3)
    d = 2.0 * un - 1.0
    d = d / np.sqrt((d * d).sum())
    if ((pos0 + steps * STEP_MM * d) ** 2).sum() > (pos0 ** 2).sum():       # towards the middle of the rig
        d = -d
    v, t, _ = fs.head()
    frames, pos, Rs = np.zeros((steps, n, h, w), np.uint16), [], []
    for k in range(steps):
        p = pos0 + k * STEP_MM * d
        R = render.euler_to_matrix((0.0, STEP_YAW * k, 0.0)).astype(np.float64) @ R0
        if k not in gone:
            items = [rr.instance(f, m, Rc, tc, head=hd) for f, m, Rc, tc, _, hd in vs.view_items(p, R, V[lead:], u[lead:])]
            frames[k, lead:] = rr.render([(v, t), fs.torso()], items, 3, w, h, K, noise=2, holes=0.02, seed=seed * 100 + k)[0]
        pos.append(p); Rs.append(R)
    out = (frames, Ks, V, u, np.stack(pos), np.stack(Rs))
    for a in out:
        a.setflags(write=False)
    return out


# ---- scripts: what both test files run, step after step.  A script is a dict: Ks, V, u, rig_begin, flags, prm (keyword
# arguments of the params), w, h, pos, Rs (the truth per step) and steps, each a dict of frames [n, h, w], inputs (rig_inputs),
# present (None or a list) and fit (None or (coarse_iterations, iterations)).
def _script(seq, rig_begin, steps, flags=0, **prm):
    frames, Ks, V, u, pos, Rs = seq
    return {"Ks": Ks, "V": V, "u": u, "rig_begin": rig_begin, "flags": flags, "prm": prm, "w": frames.shape[3], "h": frames.shape[2],
            "pos": pos, "Rs": Rs, "steps": steps}


def _step(seq, k, items, n_rigs=1, present=None, fit=None):
    return {"frames": seq[0][k], "inputs": rig_inputs(seq[0].shape[1], n_rigs, items), "present": present, "fit": fit}


def _one(seq, k, seed, pid=7, views=0b111, best=None, first=0, g=0, offset_mm=60.0):
    best = k % 3 if best is None else best
    return (g,) + person(seq[4][k], seq[5][k], seq[2], seq[3], first, views, best, pid, seed * 100 + k, offset_mm)


@functools.lru_cache(maxsize=None)
def script(name, seed=9000, motion=0):
    if name == "carried":            # detected once, then carried; the person's best camera changes every step
        seq = sequence(seed)
        return _script(seq, [0, 3], [_step(seq, k, [_one(seq, k, seed)]) for k in range(8)], flags=motion)
    if name == "absent":             # camera 1 absent in step 2; the whole rig absent in steps 4 and 5; back in 6
        seq = sequence(seed)
        pres = {2: [1, 0, 1], 4: [0, 0, 0], 5: [0, 0, 0]}
        return _script(seq, [0, 3], [_step(seq, k, [_one(seq, k, seed, best=0)], present=pres.get(k)) for k in range(7)], flags=motion)
    if name == "coast":              # seen by cameras 0 and 1 only; then unseen with only camera 2 present, beyond max_coast; then back
        seq = sequence(seed)
        steps = [_step(seq, k, [_one(seq, k, seed, views=0b011, best=k % 2)]) for k in range(2)]
        steps += [_step(seq, k, [], present=[0, 0, 1]) for k in range(2, 5)]
        steps += [_step(seq, k, [_one(seq, k, seed, views=0b011, best=0)]) for k in range(5, 7)]
        return _script(seq, [0, 3], steps, max_coast=2)
    if name == "gone":               # an empty frame in step 3: rejected, the id kept, and a start from the detection in step 4
        seq = sequence(seed, gone=(3,))
        return _script(seq, [0, 3], [_step(seq, k, [_one(seq, k, seed)]) for k in range(6)])
    if name == "unseen":             # no person record in steps 2 and 3: followed by the model; step 4 is empty: rejected and freed
        seq = sequence(seed, gone=(4,))
        steps = [_step(seq, k, [_one(seq, k, seed)] if k < 2 or k == 5 else []) for k in range(6)]
        return _script(seq, [0, 3], steps)
    if name == "jump":               # the person record of step 2 lies 200 mm off: BAD_JUMP on a carried start, FITTED again in step 3
        seq = sequence(seed, steps=6)
        steps = [_step(seq, k, [_one(seq, k, seed, offset_mm=200.0 if k == 2 else 60.0)]) for k in range(6)]
        return _script(seq, [0, 3], steps)
    if name == "unbound":            # persons 0 (id 0) and 2 (the id person 1 holds) are unbound; one of them names no head in step 1
        seq = sequence(seed, steps=6)
        steps = []
        for k in range(3):
            items = [_one(seq, k, seed, pid=0, best=0), _one(seq, k, seed + 1, pid=5, best=1), _one(seq, k, seed + 2, pid=5, best=2)]
            st = _step(seq, k, items)
            if k == 1:
                st["inputs"][3][0, 0]["best_head"] = MAX_HEADS          # names no head: ignored altogether
            steps.append(st)
        return _script(seq, [0, 3], steps)
    if name == "two_rigs":           # camera 0 is a rig of its own that sees nothing; the head's rig begins at camera 1
        seq = sequence(seed, steps=6, lead=1)
        pres = {3: [0, 1, 1, 1], 4: [1, 0, 0, 0]}
        steps = [_step(seq, k, [_one(seq, k, seed, first=1, g=1)], n_rigs=2, present=pres.get(k)) for k in range(6)]
        return _script(seq, [0, 1, 4], steps, flags=motion)
    if name == "full":               # sixteen ids fill the entries (the sixteenth is rejected: 200 mm off); then a seventeenth
        seq = sequence(seed, steps=3, w=96, h=96)
        first = [_one(seq, 0, seed + i, pid=i + 1, views=1 << (i % 3), best=i % 3, offset_mm=200.0 if i == 15 else 10.0) for i in range(16)]
        second = [_one(seq, 1, seed, pid=17, offset_mm=10.0), _one(seq, 1, seed + 1, pid=3, offset_mm=10.0)]
        third = [_one(seq, 2, seed, pid=18, offset_mm=10.0)]
        return _script(seq, [0, 3], [_step(seq, 0, first, fit=(1, 3)), _step(seq, 1, second, fit=(1, 3)), _step(seq, 2, third, fit=(1, 3))],
                       max_jump=100.0)
    raise KeyError(name)
