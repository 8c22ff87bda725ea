"""Meshes and scenes shared by the subject-set tests (test_subjects_ref.py on the CPU, test_gpu_subjects.py on the GPU; DESIGN.md
section 25): meshes whose size or corner lists are the point, seeded fields, a mesh that deforms to a zero normal, and three
subjects of tests/shape_scenes.py in one batch of frames.  What is expensive is computed once."""
import functools

import numpy as np

import shape_ref as sr
import shape_scenes as ss
import subjects_ref as sb
from depthhead_amd import fit, synth

W, H = 160, 120


def fan_mesh(spokes=300):
    """A cone whose apex, vertex 0, lies in `spokes` triangles: the longest corner list a test sums."""
    ang = 2.0 * np.pi * np.arange(spokes) / spokes
    rim = np.stack([60.0 * np.cos(ang), 60.0 * np.sin(ang), np.zeros(spokes)], axis=1)
    verts = np.concatenate([[[0.0, 0.0, -35.0]], rim]).astype(np.float32)
    tris = np.array([(0, 1 + (i + 1) % spokes, 1 + i) for i in range(spokes)], np.uint32)
    return verts, tris


def seeded_fields(verts, nk, seed):
    """nk displacement fields of up to +-20 mm a component, seeded."""
    u = synth.SplitMix(seed).uniform(nk * verts.size).reshape(nk, len(verts), 3)
    return (40.0 * u - 20.0).astype(np.float32)


def lathe_mesh(rings, segs):
    """A closed ellipsoid of 2 + rings * segs vertices: two poles, each in `segs` triangles, and `rings` rings of `segs` vertices
    between them; wound outward."""
    verts = [(0.0, 0.0, -95.0)]
    for r in range(rings):
        th = np.pi * (r + 1) / (rings + 1)
        for s in range(segs):
            ph = 2.0 * np.pi * s / segs
            verts.append((75.0 * np.sin(th) * np.cos(ph), 105.0 * np.sin(th) * np.sin(ph), -95.0 * np.cos(th)))
    verts.append((0.0, 0.0, 95.0))
    last = len(verts) - 1
    ring = lambda r, s: 1 + r * segs + s % segs
    tris = []
    for s in range(segs):
        tris.append((0, ring(0, s + 1), ring(0, s)))
        for r in range(rings - 1):
            tris += [(ring(r, s), ring(r, s + 1), ring(r + 1, s + 1)), (ring(r, s), ring(r + 1, s + 1), ring(r + 1, s))]
        tris.append((last, ring(rings - 1, s), ring(rings - 1, s + 1)))
    return np.array(verts, np.float32), np.array(tris, np.uint32)


def collapsing_disc():
    """(verts, tris, basis [1, n, 3], hub): a shallow cone facing the camera (-z) -- a hub, six rim vertices around it and an outer
    ring of six -- in integer coordinates, and ONE field that carries the rim onto the hub at coefficient 0.25, exactly: there
    the hub's six triangles are points and its normal is zero, while every other vertex keeps a triangle with area."""
    hexa = [(16, 0), (8, 14), (-8, 14), (-16, 0), (-8, -14), (8, -14)]
    hub = (0.0, 0.0, -4.0)
    rim = [(x, y, 0.0) for x, y in hexa]
    outer = [(4.0 * x, 4.0 * y, 8.0) for x, y in hexa]
    verts = np.array([hub] + rim + outer, np.float32)
    tris = []
    for i in range(6):
        j = (i + 1) % 6
        tris += [(0, 1 + j, 1 + i), (1 + i, 7 + j, 7 + i), (1 + i, 1 + j, 7 + j)]
    B = np.zeros((1, len(verts), 3), np.float32)
    B[0, 1:7] = 4.0 * (verts[0] - verts[1:7])
    return verts, np.array(tris, np.uint32), B, 0


VARIATIONS = (ss.C_TRUE, (0.00, 0.01, -0.02, 0.0), (0.12, -0.10, 0.02, 0.05))      # section 20's subject, and two within +-0.08 of it
SEEDS = (12, 13, 14)


@functools.lru_cache(maxsize=None)
def three_subjects():
    """(frames [24, H, W], K, starts [24], subject_of [24]): subject s is VARIATIONS[s] at the eight poses of seed SEEDS[s]."""
    frames, starts, who = [], [], []
    for s, (c_true, seed) in enumerate(zip(VARIATIONS, SEEDS)):
        f, K, pos, Rs = ss.subject(W, H, seed, c_true=c_true)
        frames.append(f)
        for inst in ss.rough_instances(seed, pos, Rs):
            starts.append(dict(inst, frame=inst["frame"] + 8 * s))
            who.append(s)
    return np.concatenate(frames), K, starts, who


@functools.lru_cache(maxsize=None)
def alone(s, rounds=6):
    """shape_ref.adapt of subject s by itself."""
    v, t, _, B = ss.generic()
    frames, K, pos, Rs = ss.subject(W, H, SEEDS[s], c_true=VARIATIONS[s])
    return sr.adapt(frames, K, v, t, B, ss.rough_instances(SEEDS[s], pos, Rs), fit.vertex_normals, rounds=rounds)


@functools.lru_cache(maxsize=None)
def together(rounds=6):
    v, t, _, B = ss.generic()
    frames, K, starts, who = three_subjects()
    return sb.adapt_subjects(frames, K, sb.Set(v, t, B, 3), starts, who, rounds=rounds)
