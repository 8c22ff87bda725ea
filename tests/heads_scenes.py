"""Placed scenes for the several-heads calls: frames whose votes land where the definition is decided.

TEST INFRASTRUCTURE ONLY, shared by tests/test_heads_scenes.py (CPU: the restatement of tests/heads_ref.py from both sources of
taps) and tests/test_gpu_heads_edges.py (the kernels against that restatement).

The construction.  Frames are 160 x 120 with synth.default_intrinsic (fx = 140, cx = 80, cy = 60) and 8 x 8 windows at stride
4.  A forest is depth-keyed: every split compares the 1 x 1 rectangle at the window centre with a rectangle of zero area, so a
window's leaf is chosen by the depth of its centre pixel alone, and each tree has a leaf of its own for every placed pixel.
A placed pixel sits alone at a window centre, with a depth of its own: it is one voting window, and its leaf's offsets are
p3 - (target + 1/2) in f32, so that every vote lands in the integer cell the scene names (`Builder.window`).  The three other
windows that contain the pixel have a background centre; their leaf's offsets have a positive z, so they vote behind the
camera and are dropped -- hit records that cast no position vote.  At depth 1400 a guess-grid cell is 80 x 60 mm and every
vote cluster is alone in its mean-shift window (a mode is the cell that was named); at depth 140 a cell is 8 x 6 mm, so seeds
three cells apart can be 20 or 21 mm apart.

Every scene returns a `Scene`; `reach(results, infos)` asserts that the edge is met and names what it decided.  `results` maps
(max_heads, radius) to (n_heads [n], HEAD_DTYPE [n, max_heads]) -- the restatement's or the kernels' -- and `infos` (the
restatement only) maps it to the per-frame `info` of heads_ref.heads_from_hits with "fh" and "kept" added.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable

import numpy as np

from depthhead_amd import synth
from depthhead_amd.forest import NODE_DTYPE, Forest
from oracle import pyref

import heads_ref as hr
import support_ref as sr

W, H = 160, 120
R_MAX = (1 << 31) - 1
MODEL = synth.ModelParams(stepwidth=4, subimage_width=8, subimage_height=8)
ROTS = ((0.0, 0.0, 0.0), (3.0, 0.0, 0.0))
ROTS_WIDE = ((0.0, 0.0, 0.0), (90.0, 0.0, 0.0))          # trace of the covariance 4050 > 400: no rotation vote


def one_leaf_forest(offsets, rots=ROTS):
    """One tree whose every non-zero window reaches leaf 0 (prob 1, the given offsets and rotations: at least two of each, or
    the covariance gates read NaN)."""
    nodes = np.zeros(1, dtype=NODE_DTYPE)
    nodes[0]["r1"] = (0, 0, 1, 1)
    nodes[0]["r2"] = (0, 0, 1, 1)
    nodes[0]["threshold"] = -1.0
    nodes[0]["child_zero"] = ~1
    nodes[0]["child_one"] = ~0
    offs = np.vstack([np.asarray(offsets, np.float32).reshape(-1, 3), [[0, 0, 0]]]).astype(np.float32)
    rr = np.vstack([np.asarray(rots, np.float64).reshape(-1, 3), [[0, 0, 0]]])
    k, q = len(offsets), len(rots)
    return Forest(np.array([0], np.int32), nodes, np.array([1.0, 0.0]), np.array([0, k, k + 1], np.uint32),
                  np.array([0, q, q + 1], np.uint32), offs, rr)


@dataclass
class Scene:
    forest: Forest
    model: synth.ModelParams
    frames: np.ndarray                 # uint16 [n, h, w]
    K: np.ndarray                      # float32 [3, 3]
    max_heads: tuple
    radii: tuple
    reach: Callable = field(default=lambda results, infos=None: {})

    def runs(self):
        return [(mh, r) for mh in self.max_heads for r in self.radii]


def more_trees(forest: Forest, copies: int) -> Forest:
    """The forest with its tree set `copies` times over (nodes and leaves copied too: dh_forest_create refuses a node or a
    subtree that two trees share): every count, moment and mass is multiplied by `copies`, so every tie, centroid and order
    stays."""
    nn, nl = forest.n_nodes, forest.n_leaves
    roots, nodes = [], []
    for c in range(copies):
        move = lambda v: np.where(v >= 0, v + c * nn, v - c * nl)          # noqa: E731  (~leaf - c nl == ~(leaf + c nl))
        nd = forest.nodes.copy()
        nd["child_zero"], nd["child_one"] = move(nd["child_zero"]), move(nd["child_one"])
        nodes.append(nd)
        roots.append(move(forest.roots))
    begin = lambda b, k: np.concatenate([[0], np.cumsum(np.tile(np.diff(b.astype(np.int64)), copies))]).astype(np.uint32)   # noqa: E731
    return Forest(np.concatenate(roots), np.concatenate(nodes), np.tile(forest.leaf_prob, copies), begin(forest.off_begin, copies),
                  begin(forest.rot_begin, copies), np.tile(forest.offsets, (copies, 1)), np.tile(forest.rotations, (copies, 1)))


# ---------------------------------------------------------------------------------------------------- the builder
BEHIND = None                                       # a vote behind the camera, as a target


def leaf(targets, rots=ROTS, prob=1.0, gate=True):
    """A leaf of one placed window: its votes' integer cells in order (BEHIND for a vote behind the camera); `gate`: whether
    its offsets are to pass the covariance gate."""
    assert len(targets) >= 2 and len(rots) >= 2
    return dict(targets=list(targets), rots=np.asarray(rots, np.float64).reshape(-1, 3), prob=float(prob), gate=gate)


NO_VOTE = leaf([BEHIND, BEHIND])


def px(x, y, tz=140):
    """The integer cell at depth tz that projects to pixel (x, y) (exactly at tz = 140)."""
    return (int(np.floor((x - 80) * tz / 140.0)), int(np.floor((y - 60) * tz / 140.0)), int(tz))


def cell(gx, gy, tz=1400):
    """A cell at depth tz that projects to the middle of guess-grid cell (gx, gy)."""
    return px(8 * gx + 4, 6 * gy + 3, tz)


class Builder:
    def __init__(self, n_trees=1):
        self.T = n_trees
        self.K = synth.default_intrinsic(W, H)
        assert self.K[0, 0] == 140 and self.K[0, 2] == 80 and self.K[1, 2] == 60
        self.intr = pyref.Intrinsic(self.K)
        self.wins = []                              # (frame, x, y, depth, [leaf per tree])
        self.n_frames = 0
        self.slot = 0

    def frame(self):
        self.n_frames += 1
        self.slot = 0
        return self.n_frames - 1

    def window(self, *leaves):
        """One placed pixel in the current frame, at the next free window centre (8 pixels apart) and with the next free
        depth; leaves: one per tree, NO_VOTE for the trees left out."""
        leaves = list(leaves) + [NO_VOTE] * (self.T - len(leaves))
        assert len(leaves) == self.T and self.n_frames > 0
        x, y = 4 + 8 * (self.slot % 19), 4 + 8 * (self.slot // 19)
        assert y <= 108
        self.slot += 1
        self.wins.append((self.n_frames - 1, x, y, 40 + 3 * len(self.wins), leaves))

    def _offsets(self, x, y, z, lf):
        with np.errstate(all="ignore"):
            p3 = np.array(self.intr.img_to_space([pyref.F32(x), pyref.F32(y)], pyref.F32(z)), np.float32)
        first = next((t for t in lf["targets"] if t is not None), (0, 0, 0))
        out = []
        for t in lf["targets"]:
            if t is None:
                want = np.array([first[0], first[1], -1.0])
            else:
                assert t[2] >= 0
                want = np.array([c + 0.5 if c >= 0 else c - 0.5 for c in t])
            out.append((p3 - want.astype(np.float32)).astype(np.float32))
        offs = np.stack(out)
        d = p3[None, :] - offs                                          # prediction.rs:647, in f32
        for t, dd in zip(lf["targets"], d):
            if t is None:
                assert dd[2] < 0
            else:
                assert not dd[2] < 0 and tuple(sr.as_i32_vec(dd)) == tuple(t), (t, dd)
        passes = bool(pyref.trace_of_cov([tuple(o) for o in offs], pyref.F32) <= pyref.MAX_VARIANCE_OFFSET)
        assert passes == lf["gate"], (lf["targets"], passes)
        return offs

    def build(self):
        frames = np.zeros((self.n_frames, H, W), np.uint16)
        z = [0] + [wn[3] for wn in self.wins]
        m = len(z)
        nodes, roots = [], []
        prob, n_off, n_rot, offs, rots = [], [], [], [], []

        def tree(lo, hi, base):
            if lo == hi:
                return ~(base + lo)
            mid = (lo + hi) // 2
            i = len(nodes)
            nodes.append(None)
            zero, one = tree(lo, mid, base), tree(mid + 1, hi, base)
            nodes[i] = ((4, 4, 5, 5), (0, 0, 0, 0), z[mid + 1] - 0.5, zero, one)
            return i
        for t in range(self.T):
            roots.append(tree(0, m - 1, t * m))
            # leaf t * m: the background centre (p3 = 0): two votes behind the camera, rotation votes of its own
            prob.append(1.0); n_off.append(2); n_rot.append(2)
            offs.append(np.array([[0, 0, 50], [0, 0, 51]], np.float32)); rots.append(np.asarray(ROTS, np.float64))
            for f, x, y, depth, leaves in self.wins:
                lf = leaves[t]
                prob.append(lf["prob"]); n_off.append(len(lf["targets"])); n_rot.append(len(lf["rots"]))
                offs.append(self._offsets(x, y, depth, lf)); rots.append(lf["rots"])
        for f, x, y, depth, _ in self.wins:
            frames[f, y, x] = depth
        nd = np.zeros(len(nodes), dtype=NODE_DTYPE)
        for i, n in enumerate(nodes):
            nd[i] = n
        ob = np.concatenate([[0], np.cumsum(n_off)]).astype(np.uint32)
        rb = np.concatenate([[0], np.cumsum(n_rot)]).astype(np.uint32)
        forest = Forest(np.array(roots, np.int32), nd, np.array(prob), ob, rb, np.concatenate(offs), np.concatenate(rots))
        return forest, frames, self.K


# ---------------------------------------------------------------------------------------------------- what reach reads
def mids(results, key, frame):
    """The heads of one frame as a list of integer (x, y, z) midpoints, in the order of the records."""
    n, recs = results[key]
    return [tuple(int(v) for v in sr.as_i32_vec(recs[frame, j]["pose"]["mid_point"])) for j in range(int(n[frame]))]


def masses(results, key, frame):
    n, recs = results[key]
    return [int(recs[frame, j]["support"]["mass"]) for j in range(int(n[frame]))]


def unused_slots_zero(results):
    for (mh, r), (n, recs) in results.items():
        for i in range(len(n)):
            assert recs[i, int(n[i]):].tobytes() == bytes((mh - int(n[i])) * recs.dtype.itemsize), (mh, r, i)
    return True


def hit_masks(info, radius):
    """Per hit record of a frame, the bit mask of the candidates (seed order) one of whose cubes holds one of its votes."""
    fh = info["fh"]
    out = {}
    for c in info["candidates"]:
        m = np.array(c["mid"], np.int64)
        inside = np.all(np.abs(fh["cells"] - m[None, :]) <= int(radius), axis=1) if len(fh["cells"]) else np.zeros(0, bool)
        for hit in np.unique(fh["hit"][inside]):
            out[int(hit)] = out.get(int(hit), 0) | 1 << c["k"]
    return out


def differ(results, a, b):
    return results[a][0].tobytes() != results[b][0].tobytes() or results[a][1].tobytes() != results[b][1].tobytes()


# ---------------------------------------------------------------------------------------------------- 1. seed order
def seed_order() -> Scene:
    """k_heads_seeds: the key count << 32 | ~index and the Chebyshev test `<= DH_HEADS_SUPPRESS`.  Every vote at depth 1400,
    where each cluster is alone: the heads are the picked cells' own votes.  A leaf of k equal offsets puts k * (1000 // k)
    into its cell: 1000 (k = 2), 999 (3), 996 (6), 994 (7), 990 (11), 988 (13).
    frame 0: the four corner cells 0, 19, 380, 399 at 1000 each (cell 0 reached through the clamp from left of and above the
             frame, 399 from right of and below it) and cell 210 at 999: a tie for the first pick, and max_heads 1 .. 4 cut
             the walk after cell 0, 19, 380, 399;
    frame 1: A = (10, 10) at 2000; 2 cells from it B = (12, 10) at 1000, D = (10, 12) at 994, F = (12, 12) at 990 (dropped);
             3 cells from it C = (13, 10) at 999, E = (10, 13) at 996, G = (13, 13) at 988 (picked, in that order);
    frame 2: three seeds on the borders (cells 10, 200, 219), fewer than max_heads = 4;  frame 3: one seed;  frame 4: empty."""
    b = Builder()
    two = lambda t: leaf([t, t])                                  # noqa: E731
    many = lambda t, k: leaf([t] * k)                             # noqa: E731
    b.frame()
    corners = [px(-30, -25, 1400), cell(19, 0), cell(0, 19), px(200, 170, 1400)]
    for t in corners:
        b.window(two(t))
    b.window(many(cell(10, 10), 3))
    b.frame()
    A, B, C, D, E, F, G = (cell(10, 10), cell(12, 10), cell(13, 10), cell(10, 12), cell(10, 13), cell(12, 12), cell(13, 13))
    b.window(two(A)); b.window(two(A)); b.window(two(B)); b.window(many(C, 3)); b.window(many(D, 7)); b.window(many(E, 6))
    b.window(many(F, 11)); b.window(many(G, 13))
    b.frame()
    borders = [cell(10, 0), cell(0, 10), cell(19, 10)]
    b.window(two(borders[0])); b.window(two(borders[0])); b.window(two(borders[1])); b.window(many(borders[2], 3))
    b.frame()
    b.window(two(cell(7, 3)))
    b.frame()
    forest, frames, K = b.build()
    radii = (30,)

    def reach(results, infos=None):
        if infos is not None:
            for mh in (1, 2, 3, 4):
                fr = infos[(mh, 30)]
                assert fr[0]["picks"] == [0, 19, 380, 399][:mh], fr[0]["picks"]
                assert [int(fr[0]["grid"][c]) for c in (0, 19, 380, 399, 210)] == [1000, 1000, 1000, 1000, 999]
                assert fr[1]["picks"] == [210, 213, 270, 273][:mh], fr[1]["picks"]
                assert [int(fr[1]["grid"][c]) for c in (210, 212, 213, 250, 270, 252, 273)] == [2000, 1000, 999, 994, 996, 990, 988]
                assert fr[2]["picks"] == [10, 200, 219][:mh] and fr[3]["picks"] == [67] and fr[4]["picks"] == []
                assert all(f["merged"] == 0 for f in fr)
        for mh in (1, 2, 3, 4):
            key = (mh, 30)
            assert mids(results, key, 0) == corners[:mh], mids(results, key, 0)        # equal masses: seed order
            assert masses(results, key, 0) == [1000] * mh
            assert set(mids(results, key, 1)) == set([A, C, E, G][:mh]), mids(results, key, 1)
            assert mids(results, key, 2) == borders[:mh] and mids(results, key, 3) == [cell(7, 3)] and mids(results, key, 4) == []
        return {"equal counts, lower index first, the first pick too": True, "suppressed at 2 cells, picked at 3 (x, y, diagonal)": True,
                "corner and border seed cells": True, "max_heads 1 to 4 cut the walk at different cells": True,
                "fewer seeds than max_heads": True, "equal masses in seed order": True, "unused slots zero": unused_slots_zero(results)}
    return Scene(forest, MODEL, frames, K, (1, 2, 3, 4), radii, reach)


# ---------------------------------------------------------------------------------------------------- 2. moments
def moments() -> Scene:
    """k_heads_moments: the per-lane run (`cur`) and `flush`, and floor_div_i128 on negative sums.  Depth 140 / 141, left of
    and above the principal point, so x and y are negative.  Two trees.
    Window 0, tree 0: twelve offsets (valtoadd 83) in the order a a' b n - b' a - n b a' b', with a, a' in seed cell SA = (2, 2),
    b, b' in seed cell SB = (6, 6), n in (3, 2) (within two cells of SA: no seed) and `-` behind the camera.
    Window 1 (three offsets, valtoadd 333, both trees) votes into SA as well; window 2 (valtoadd 500) into SB.
    SA's centroid is negative with a remainder on x and y; SB's is negative and divides exactly.  The model runs zero mean-shift
    iterations, so each head's midpoint is its seed and the records themselves show the floor."""
    b = Builder(2)
    a, a2, n_ = (-60, -45, 140), (-61, -46, 141), (-52, -45, 140)
    sb, sb2 = (-30, -20, 140), (-28, -18, 140)
    b.frame()
    b.window(leaf([a, a2, sb, n_, BEHIND, sb2, a, BEHIND, n_, sb, a2, sb2]))
    b.window(leaf([(-59, -44, 140)] * 3), leaf([(-59, -44, 140)] * 3))
    b.window(leaf([sb, sb2]))
    forest, frames, K = b.build()

    def reach(results, infos=None):
        met = {"unused slots zero": unused_slots_zero(results)}
        if infos is not None:
            info = infos[(4, 30)][0]
            fh = info["fh"]
            assert info["picks"] == [2 * 20 + 2, 6 * 20 + 6], info["picks"]
            assert int(info["grid"][2 * 20 + 3]) == 2 * 83                         # the non-seed cell holds votes
            # one hit whose votes alternate: its cells in order visit SA, SB, the non-seed cell, SA again ...
            h0 = fh["g"][fh["hit"] == 0].tolist()
            assert h0 == [42, 42, 126, 43, 126, 42, 43, 126, 42, 126], h0           # (two of twelve behind the camera)
            rem = []
            for c in info["candidates"]:
                sel = fh["g"] == c["seed_cell"]
                sv = int(fh["vals"][sel].sum())
                sums = [hr.exact_sum(fh["vals"][sel], fh["cells"][sel, q]) for q in range(3)]
                rem.append([s % sv for s in sums])
                assert all(s // sv == c["seed"][q] for q, s in enumerate(sums))
                assert sums[0] < 0 and sums[1] < 0
            assert rem[0][0] != 0 and rem[0][1] != 0, rem                          # floor and truncation differ on x and y
            assert rem[1] == [0, 0, 0], rem                                        # divides exactly
            assert info["candidates"][1]["seed"] == (-29, -19, 140)
            assert len(set(fh["vals"][fh["g"] == 42].tolist())) == 2 and len(set(fh["hit"][fh["g"] == 42].tolist())) == 3
            met.update({"a hit alternating between two seed cells, a non-seed cell and behind the camera": True,
                        "negative centroid with a remainder on x and y": True, "negative centroid dividing exactly": True,
                        "several hits and valtoadd in one seed cell": True})
        assert set(mids(results, (4, 30), 0)) == {(-60, -45, 140), (-29, -19, 140)}, mids(results, (4, 30), 0)
        assert mids(results, (1, 30), 0) == [(-60, -45, 140)]                      # -59.2 and -44.2 floor to -60 and -45
        met["the floor of a negative centroid in the records"] = True
        return met
    model = synth.ModelParams(stepwidth=4, subimage_width=8, subimage_height=8, meanshift_iterations=0)
    return Scene(forest, model, frames, K, (4, 1), (30,), reach)


# ---------------------------------------------------------------------------------------------------- 3. cubes
R_STAR = 12


def cubes() -> Scene:
    """k_heads_support: both compares of each face of each cube, head masks with several bits, the rotation gate.  Depth 140,
    two trees.  Heads H0 = (4, 3, 140), H1 = H0 + (24, 0, 0), H2 = H0 + (12, 24, 0): three seed cells, modes more than 20
    apart, cubes that overlap at r* = 12 (the cell H0 + (12, 12, 0) lies in all three; H0 + (12, 0, 0) in H0's and H1's).
    Each head: two windows on its mode; for each axis and sign one window voting at mid +- r* (inside at r*, outside at
    r* - 1) and mid +- (r* + 1) (outside at both).  These sit outside the mean-shift window (-10 .. 9) of the mode and within
    two guess cells of it, so they are no seeds and move no mode.  One face window's leaf fails the rotation gate; one window
    passes the rotation gate and fails the offset gate (rotation votes in the plain call, none here)."""
    b = Builder(2)
    H0 = (4, 3, 140)
    heads = [H0, (H0[0] + 24, H0[1], 140), (H0[0] + 12, H0[1] + 24, 140)]
    hrots = [((10.0, 0.0, 0.0), (11.0, 0.0, 0.0)), ((-20.0, 5.0, 0.0), (-21.0, 5.0, 0.0)), ((0.0, 30.0, 0.0), (0.0, 31.0, 0.0))]
    b.frame()
    for hd, rr in zip(heads, hrots):
        b.window(leaf([hd, hd], rr), leaf([hd, hd], rr))          # both trees: windows once, hits once per tree
        b.window(leaf([hd, hd], rr))
    first = True
    for hd, rr in zip(heads, hrots):
        for q in range(3):
            for s in (1, -1):
                t_in, t_out = list(hd), list(hd)
                t_in[q] += s * R_STAR
                t_out[q] += s * (R_STAR + 1)
                b.window(leaf([tuple(t_in), tuple(t_out)], ROTS_WIDE if first else rr))
                first = False
    b.window(leaf([(H0[0] + 12, H0[1] + 12, 140)] * 2, hrots[2]))           # in all three cubes at r*
    b.window(leaf([(0, 0, 140), (300, 0, 140)], ((40.0, 40.0, 40.0), (41.0, 40.0, 40.0)), gate=False))
    forest, frames, K = b.build()
    radii = (R_STAR, R_STAR - 1, 0, R_MAX, 30)

    def reach(results, infos=None):
        met = {"unused slots zero": unused_slots_zero(results)}
        assert sorted(mids(results, (4, R_STAR), 0)) == sorted(heads), mids(results, (4, R_STAR), 0)
        for mh in (4, 2):
            assert differ(results, (mh, R_STAR), (mh, R_STAR - 1))
        # at r* every face vote counts; at r* - 1 none; at 0 only the mode's own cell; at 2^31 - 1 every vote of the frame
        n, recs = results[(4, R_MAX)]
        assert all(int(recs[0, j]["support"]["mass"]) == int(recs[0, j]["support"]["total_mass"]) for j in range(int(n[0])))
        assert sorted(masses(results, (4, 0), 0)) == [3000, 3000, 3000]
        assert sorted(masses(results, (4, R_STAR - 1), 0)) == [3000, 3500, 3500]      # + the faces of the other cubes inside
        met["r* against r* - 1 decided"] = True
        met["radius 0 and 2^31 - 1"] = True
        if infos is not None:
            info = infos[(4, R_STAR)][0]
            fh = info["fh"]
            assert info["merged"] == 0 and len(info["candidates"]) == 3
            for c in info["candidates"]:
                m = np.array(c["mid"], np.int64)
                d = fh["cells"] - m[None, :]
                for q in range(3):
                    others = [k for k in range(3) if k != q]
                    alone = np.all(d[:, others] == 0, axis=1)
                    for s in (1, -1):
                        assert (alone & (d[:, q] == s * R_STAR)).any() and (alone & (d[:, q] == s * (R_STAR + 1))).any(), (c["k"], q, s)
            mk = hit_masks(info, R_STAR)
            bits = [bin(v).count("1") for v in mk.values()]
            assert 2 in bits and 3 in bits, bits
            # hits per window: the mode windows of both trees
            n4, recs4 = results[(4, 0)]
            assert all(int(recs4[0, j]["support"]["hits"]) == 3 and int(recs4[0, j]["support"]["windows"]) == 2 for j in range(3))
            rot_hits = set(fh["rot_hit"].tolist())
            sup_hits = set(mk)
            assert sup_hits - rot_hits, "no supporting hit whose leaf fails the rotation gate"
            assert rot_hits - set(fh["hit"].tolist()), "no rotation-voting hit without a position vote"
            met.update({"a vote on each face of each cube, and one cell outside it": True, "a hit supporting two and three heads": True,
                        "a supporting hit that fails the rotation gate": True, "a rotation-voting hit without a position vote": True,
                        "several trees on one window": True})
        return met
    return Scene(forest, MODEL, frames, K, (4, 2), radii, reach)


# ---------------------------------------------------------------------------------------------------- 4. finish
def finish() -> Scene:
    """k_heads_finish: `d <= DH_MEANSHIFT_KERNEL_SIZE`, merging against kept heads only, the stable sort by mass.  Depth 140
    (70 / 90 for z), every mode one cell of its own.  The first head of a frame has two windows, so it is the first seed.
    frames 0 / 1: 20 / 21 apart on x;  2 / 3: on y;  4 / 5: on z (15 apart on y, so that the seed cells differ);
    frame 6: (20, 20, 20) apart (merged: Chebyshev, not Euclidean);
    frame 7: a chain A, B = A + (20, 0, 0) (merged), C = B + (20, 20, 0) (20 from B, 40 from A: kept);
    frame 8: X with seed count 2000 and Y with 1000 whose cube at r = 12 holds three further clusters of 999: the mass order
             reverses the seed order at r = 12 and follows it at r = 0;
    frame 9: two equal votes three cells apart on x in one seed cell: the mode is the empty cell between them, so at r = 0 the
             head has a seed and no mass and the frame, which is not empty, ends with no head."""
    b = Builder()
    two = lambda t: leaf([t, t])                                  # noqa: E731
    pairs = []
    for q, base, other in ((0, (7, 5, 140), None), (1, (7, 5, 140), None), (2, (0, 0, 70), (0, 15, 90))):
        for dist in (20, 21):
            t = list(base if other is None else other)
            if other is None:
                t[q] += dist
            else:
                t[2] = base[2] + dist
            b.frame()
            b.window(two(base)); b.window(two(base)); b.window(two(tuple(t)))
            pairs.append((base, tuple(t)))
    b.frame()
    b.window(two((7, 5, 140))); b.window(two((7, 5, 140))); b.window(two((27, 25, 160)))
    b.frame()
    A, B, C = (7, 5, 140), (27, 5, 140), (47, 25, 140)
    b.window(two(A)); b.window(two(A)); b.window(two(B)); b.window(leaf([C] * 3))
    b.frame()
    X, Y = (-50, -30, 140), (30, 20, 140)
    b.window(two(X)); b.window(two(X)); b.window(two(Y))
    for dq in ((12, 0, 0), (-12, 0, 0), (0, 12, 0)):
        b.window(leaf([tuple(Y[k] + dq[k] for k in range(3))] * 3))
    b.frame()
    b.window(leaf([(8, 2, 140), (11, 2, 140)]))
    forest, frames, K = b.build()

    def reach(results, infos=None):
        met = {"unused slots zero": unused_slots_zero(results)}
        for r in (30, 12):
            key = (4, r)
            for i, axis in enumerate("xyz"):
                assert mids(results, key, 2 * i) == [pairs[2 * i][0]], (axis, mids(results, key, 2 * i))
                assert mids(results, key, 2 * i + 1) == list(pairs[2 * i + 1]), (axis, mids(results, key, 2 * i + 1))
            assert mids(results, key, 6) == [(7, 5, 140)]
            assert mids(results, key, 7) == [A, C]
        assert mids(results, (4, 12), 8) == [Y, X] and masses(results, (4, 12), 8) == [1000 + 3 * 999, 2000]
        assert mids(results, (4, 0), 8) == [X, Y]
        assert mids(results, (1, 12), 8) == [X]
        assert int(results[(4, 0)][0][9]) == 0 and frames[9].any() and mids(results, (4, 12), 9) == [(9, 2, 140)]
        met.update({"merged at 20, kept at 21, on x, y and z": True, "merged at (20, 20, 20)": True,
                    "a chain: merging compares with kept heads only": True, "a mass order that reverses the seed order": True,
                    "a seed with mass 0 at radius 0, dropped; a non-empty frame without a head": True})
        if infos is not None:
            fr = infos[(4, 30)]
            assert [f["merged"] for f in fr[:8]] == [1, 0, 1, 0, 1, 0, 1, 1], [f["merged"] for f in fr]
            assert all(len(f["picks"]) == 2 for f in fr[:7]) and len(fr[7]["picks"]) == 3
            c = infos[(4, 0)][9]["candidates"]
            assert len(c) == 1 and c[0]["support"]["mass"] == 0 and c[0]["support"]["total_mass"] == 1000
        return met
    return Scene(forest, MODEL, frames, K, (4, 1), (30, 12, 0), reach)


# ---------------------------------------------------------------------------------------------------- 5. saturated cells
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def saturated() -> Scene:
    """Vote cells saturated at INT32_MIN / INT32_MAX: equal offsets of magnitude 2^31 pass the covariance gate (variance 0),
    which no family of tests/edge_families.py does -- there a leaf with a huge or non-finite offset fails the gate and casts no
    position vote.  The seed, the mode and the cube's faces sit on the limits of i32: floor_div_i128 on sums of -2^31 v, the
    mean shift's wrapping window, m +- r in 64 bits.
    frame 0: one head at (MAX, MIN, MAX) (guess cell 19, through the clamps);
    frame 1: a head at (MIN, MAX, 140) (cell 380) and an ordinary one in cell 210, which is the first seed."""
    b = Builder()
    b.frame()
    S0, S1, N = (I32_MAX, I32_MIN, I32_MAX), (I32_MIN, I32_MAX, 140), cell(10, 10)
    b.window(leaf([S0, S0]))
    b.frame()
    b.window(leaf([S1, S1])); b.window(leaf([N, N])); b.window(leaf([N, N]))
    forest, frames, K = b.build()

    def reach(results, infos=None):
        met = {"unused slots zero": unused_slots_zero(results)}
        for r in (0, 30, R_MAX):
            assert mids(results, (4, r), 0) == [S0] and masses(results, (4, r), 0) == [1000], (r, mids(results, (4, r), 0))
        assert mids(results, (4, 30), 1) == [N, S1] and masses(results, (4, 30), 1) == [2000, 1000]
        # m +- r in 64 bits: MIN + (2^31 - 1) = -1 < 40 and 40 - (2^31 - 1) > MIN, so even the full radius keeps the two apart
        assert masses(results, (4, R_MAX), 1) == [2000, 1000]
        if infos is not None:
            assert infos[(4, 30)][0]["picks"] == [19] and infos[(4, 30)][1]["picks"] == [210, 380]
            assert [c["seed"] for c in infos[(4, 30)][1]["candidates"]] == [N, S1] and infos[(4, 30)][0]["candidates"][0]["seed"] == S0
        met["a seed, a mode and a cube at the limits of i32"] = True
        return met
    return Scene(forest, MODEL, frames, K, (4,), (0, 30, R_MAX), reach)


SCENES = {f.__name__: f for f in (seed_order, moments, cubes, finish, saturated)}

_cache = {}


def scene(name) -> Scene:
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]


def restate(tables, sc_or_fam, frames, Ks, taps, runs, dtype):
    """(results, infos) of frames through heads_ref.heads_from_hits: taps[i] = (leaf_idx, patch_flags) of frame i seen through
    Ks[i]; runs: [(max_heads, radius)]."""
    n, h, w = frames.shape
    results, infos = {}, {}
    fhs = [hr.frame_hits(tables, sc_or_fam.model, frames[i], Ks[i], taps[i][0], taps[i][1]) for i in range(n)]
    for mh, r in runs:
        nh = np.zeros(n, np.uint32)
        recs = np.zeros((n, mh), dtype=dtype)
        infos[(mh, r)] = []
        for i in range(n):
            k, kept, info = hr.heads_from_hits(fhs[i], sc_or_fam.model, w, h, mh, r)
            nh[i] = k
            recs[i] = hr.as_records(k, kept, mh, dtype)
            info.update(fh=fhs[i], kept=kept)
            infos[(mh, r)].append(info)
        results[(mh, r)] = (nh, recs)
    return results, infos


# ---------------------------------------------------------------------------------------------------- the 3-D families
FAMILY_MAX_HEADS = 4


def family_heads(name, decoy):
    """A 3-D family of tests/edge_families.py through the restatement, from pyref's taps, once per session: dict with fam,
    frames, Ks [n, 3, 3], radii (0, DH_SUPPORT_RADIUS, 2^31 - 1, r*, r* - 1; r* as test_support_families.boundary_radius takes
    it, from the first head's midpoints), runs, results, infos and the pyref results."""
    key = ("family", name, decoy)
    if key not in _cache:
        from depthhead_amd import _lib
        from test_edge_pyref import decoy_results, family_results
        from test_support_families import boundary_radius
        fam, res = family_results(name)
        n = fam.frames.shape[0]
        Ks = np.repeat(np.asarray(fam.K, np.float32)[None], n, axis=0)
        if decoy:
            Ks, res = decoy_results(name)
        tables = sr.LeafTables(fam.forest)
        taps = [(res[i]["leaf_idx"], res[i]["patch_flags"]) for i in range(n)]
        with np.errstate(all="ignore"):
            first, infos1 = restate(tables, fam, fam.frames, Ks, taps, [(FAMILY_MAX_HEADS, _lib.SUPPORT_RADIUS)], _lib.HEAD_DTYPE)
            for i, info in enumerate(infos1[(FAMILY_MAX_HEADS, _lib.SUPPORT_RADIUS)]):
                assert np.array_equal(info["grid"], res[i]["pos_grid"].astype(np.int64)), (name, i, "guess cells against pyref's pos_grid")
            nh, recs = first[(FAMILY_MAX_HEADS, _lib.SUPPORT_RADIUS)]
            votes = [sr.frame_votes(tables, fam.model, fam.frames[i], Ks[i], *taps[i]) for i in range(n)]
            rs = boundary_radius(votes, recs[:, 0]["pose"]["mid_point"])
            radii = [0, _lib.SUPPORT_RADIUS, R_MAX, rs, rs - 1]
            runs = [(FAMILY_MAX_HEADS, r) for r in radii]
            results, infos = restate(tables, fam, fam.frames, Ks, taps, runs, _lib.HEAD_DTYPE)
        _cache[key] = dict(fam=fam, frames=fam.frames, Ks=Ks, radii=radii, runs=runs, results=results, infos=infos, res=res,
                           tables=tables)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- frames for the launch shapes
def _slot_xy(s):
    return 4 + 8 * (s % 19), 4 + 8 * (s // 19)


def cubes_variants() -> np.ndarray:
    """Five distinct frames over the forest of `cubes`: the scene's frame; without H2's two mode windows; empty; H0's mode
    windows alone; without H0's two-tree mode window."""
    f = scene("cubes").frames[0]

    def keep(slots):
        out = np.zeros_like(f)
        for s in slots:
            x, y = _slot_xy(s)
            out[y, x] = f[y, x]
        return out
    every = list(range(26))
    return np.stack([f, keep([s for s in every if s not in (4, 5)]), np.zeros_like(f), keep([0, 1]), keep(every[1:])])


def cubes_block() -> np.ndarray:
    """The frame of `cubes` with rows 24 .. 119 flat at the depth of H1's second mode window: every window centred in the block
    reaches that window's leaves, and votes where it does moved by its own centre -- several hundred voting windows on one
    frame, a few thousand hit records with the tree set doubled."""
    f = scene("cubes").frames[0].copy()
    x, y = _slot_xy(3)
    f[24:, :] = f[y, x]
    return f[None]
