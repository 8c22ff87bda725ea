"""Scenes shared by the rig subject tracker's tests (test_rig_subject_track_ref.py on the CPU, test_gpu_rig_subject_tracker.py on the
GPU): a gallery of ident_scenes' kind -- subjects that differ by one coefficient -- seen by rigs of cameras on
an arc (view_fit_scenes.arc), and per rig some people who move a little every step, each splatted from the model of the subject
it is (cheap at any size) into every camera of its rig at the composite camera pose.  What a rig tracker step would report of them
is made by hand, as rig_fit_track_scenes makes it: no forest is needed.  A stranger is a head of the same mesh at a coefficient no
subject of the gallery has.  Every scene is computed once and handed out read-only."""
import functools

import numpy as np

import ident_views_scenes as ivs
import rig_fit_track_scenes as rsc
import subject_track_scenes as sts
import subjects_ref as sb
import surface_scenes as us
import view_fit_scenes as vs
from depthhead_amd import fit, render, synth

STEP_MM, STEP_YAW = 5.0, 2.0
STRANGER = sts.STRANGER
APART = 170.0                     # mm between the people of one rig, along the world's x


class Scene:
    """frames [steps, n_cams, h, w] u16, Ks, V, u, rig_begin, and pos [steps][rig][person] / Rs alike: the truth."""

    def __init__(self, frames, Ks, V, u, rig_begin, pos, Rs, who):
        self.frames, self.Ks, self.V, self.u, self.rig_begin, self.pos, self.Rs, self.who = frames, Ks, V, u, rig_begin, pos, Rs, who
        self.n_cams, self.n_rigs = len(Ks), len(rig_begin) - 1
        self.h, self.w = frames.shape[2:]

    def item(self, k, g, j, pid, views=None, best=0, offset_mm=10.0, head=0):
        """(rig, dh_rig_person, dh_head) of person j of rig g at step k under id `pid`, seen by the cameras of `views` (None: all)."""
        c0, nc = self.rig_begin[g], self.rig_begin[g + 1] - self.rig_begin[g]
        views = (1 << nc) - 1 if views is None else views
        return (g,) + rsc.person(self.pos[k][g][j], self.Rs[k][g][j], self.V, self.u, c0, views, best, pid, 1000 * k + 10 * g + j, offset_mm, head)

    def inputs(self, items, max_heads=rsc.MAX_HEADS):
        return rsc.rig_inputs(self.n_cams, self.n_rigs, items, max_heads)


@functools.lru_cache(maxsize=None)
def scene(name, n_subjects, w, h, rigs, steps, seed=3, surface=False, gone=(), z=800.0):
    """rigs: per rig (cameras, (who of person 0, who of person 1, ...)); gone: (step, rig, person) triples that are in no frame.
    Every rig has a world of its own about which its cameras stand on an arc; its people stand APART along x."""
    v, t, B, st = sts.restated_set(name, n_subjects, surface)
    strange = sb.points(v, B, [sts.STRANGER_COEFF])
    Vs, us_, rig_begin = [], [], [0]
    for nc, _ in rigs:
        V, u = fit.views_from_rig(*vs.arc(ivs.spread(nc, 25.0), [z] * nc))
        Vs.append(V); us_.append(u)
        rig_begin.append(rig_begin[-1] + nc)
    V, u = np.concatenate(Vs), np.concatenate(us_)
    n = rig_begin[-1]
    K = synth.default_intrinsic(w, h)
    Ks = np.ascontiguousarray(np.broadcast_to(K, (n, 3, 3))).astype(np.float32)
    frames = np.zeros((steps, n, h, w), np.uint16)
    pos = [[[None] * len(people) for _, people in rigs] for _ in range(steps)]
    Rs = [[[None] * len(people) for _, people in rigs] for _ in range(steps)]
    for g, (nc, people) in enumerate(rigs):
        for j, who in enumerate(people):
            r = synth.SplitMix(910000 + 1000 * seed + 10 * g + j).uniform(6)
            rot0 = (2.0 * r[:3] - 1.0) * 8.0
            p0 = np.array([(j - 0.5 * (len(people) - 1)) * APART + 10.0 * (2.0 * r[3] - 1.0), 20.0 * (2.0 * r[4] - 1.0), 20.0 * (2.0 * r[5] - 1.0)])
            ang = 2.0 * np.pi * r[0]
            d = np.array([0.4 * np.cos(ang), 0.5 * np.sin(ang), 0.75])
            d = d / np.sqrt((d * d).sum())
            pts = strange if who == STRANGER else st.pts[who]
            for k in range(steps):
                p = p0 + k * STEP_MM * d
                rot = rot0.copy()
                rot[1] += STEP_YAW * k
                R = render.euler_to_matrix(rot).astype(np.float64)
                pos[k][g][j], Rs[k][g][j] = p, R
                if (k, g, j) in gone:
                    continue
                for c in range(rig_begin[g], rig_begin[g + 1]):
                    Rc, tc = vs.camera_pose(V[c], u[c], R, p)
                    f = us.splat(pts, K, us.instance(0, Rc, tc), w, h, seed=((seed * 100 + k) * 64 + c) * 4 + j)
                    old = frames[k, c]
                    frames[k, c] = np.where((f != 0) & ((old == 0) | (f < old)), f, old)
    frames.setflags(write=False)
    return Scene(frames, Ks, V, u, rig_begin, pos, Rs, tuple(people for _, people in rigs))
