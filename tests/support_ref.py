"""CPU restatement of the vote-support record (include/depthhead_hip.h: dh_support).

TEST INFRASTRUCTURE ONLY.  It starts from the taps of one frame (leaf_idx, patch_flags, mid_point) and the forest's leaf
tables, and replays the position votes of the reference
(prediction.rs:544-667) with pyref's f32 `Intrinsic.img_to_space` and `trace_of_cov`:

* windows past the 0.7 gate (patch_flags == 3), in the reference's loop order (window i at centre
  (lw + (i % nx) * step, lh + (i // nx) * step));
* every tree's leaf with prob > 0 whose offsets pass the covariance gate (trace <= 5200, f32);
* every offset o with p3 - o not negative in z; cell c = (as_i32(p3 - o)) (DH_ZSCALEFACTOR = 1).

A vote supports the pose when max_k |c_k - m_k| <= r, m = as_i32(mid_point).

The taps come from either restatement of the prediction: the C oracle's (`pyoracle.predict(..., taps=True)`, `support_ref`)
or pyref's result dicts (`replay`), so that a misreading shared by the oracle and the kernels cannot stay green.
`hit_boxes` restates k_forest's per-leaf offset box as k_emit turns it into each hit's HitBox, and `branches` sorts the hits
into k_support's three cases.
"""
from __future__ import annotations

import numpy as np

from oracle import pyref

SUPPORT_FIELDS = ("x", "y", "width", "height", "windows", "hits", "mass", "total_mass")


class LeafTables:
    """Per-leaf facts of a forest the votes need: valtoadd, the offset gate, the offsets as f32 [k, 3]."""

    def __init__(self, forest):
        self.forest = forest
        self._gate = {}
        self._box = {}

    def box(self, leaf: int):
        """(omin, omax) f32 [3] of a leaf's offsets, as k_forest.hip builds them: +-inf in every coordinate when some offset
        is not finite or exceeds 3e38 in magnitude."""
        if leaf not in self._box:
            f = self.forest
            offs = np.asarray(f.offsets[f.off_begin[leaf]:f.off_begin[leaf + 1]], dtype=np.float32).reshape(-1, 3)
            if not (np.abs(offs) <= np.float32(3.0e38)).all():
                lo, hi = np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32)
            else:
                lo, hi = offs.min(axis=0), offs.max(axis=0)
            self._box[leaf] = (lo, hi)
        return self._box[leaf]

    def votes(self, leaf: int):
        """(valtoadd, offsets f32 [k, 3]) of a leaf that casts position votes, else None."""
        f = self.forest
        if leaf in self._gate:
            return self._gate[leaf]
        lp = pyref.F64(f.leaf_prob[leaf])
        res = None
        if lp > 0.0:
            offs = np.asarray(f.offsets[f.off_begin[leaf]:f.off_begin[leaf + 1]], dtype=np.float32).reshape(-1, 3)
            if pyref.trace_of_cov([tuple(o) for o in offs], pyref.F32) <= pyref.MAX_VARIANCE_OFFSET:
                v = (pyref.as_usize(pyref.F64(pyref.F64(1000.0) * lp)) // len(offs)) & 0xFFFFFFFF
                res = (int(v), offs)
        self._gate[leaf] = res
        return res


def as_i32_vec(a: np.ndarray) -> np.ndarray:
    """Rust `as i32` of f32 values, element-wise (NaN -> 0, saturating)."""
    a = np.asarray(a, dtype=np.float64)
    out = np.where(np.isnan(a), 0.0, np.clip(a, -2147483648.0, 2147483647.0))
    return np.trunc(out).astype(np.int64)


def _voting_hits(tables: LeafTables, model, img, K, leaf_idx, patch_flags):
    """(window, tree, leaf, p3 f32 [3], valtoadd, offsets) of every hit record with position votes, in the reference's order."""
    img = np.asarray(img, dtype=np.uint16)
    h, w = img.shape
    nx, _ = model.patch_grid(w, h)
    lw, lh, step = int(model.subimage_width) // 2, int(model.subimage_height) // 2, int(model.stepwidth)
    intr = pyref.Intrinsic(K)
    for wi in np.flatnonzero(np.asarray(patch_flags) == 3):
        cx, cy = lw + (wi % nx) * step, lh + (wi // nx) * step
        with np.errstate(all="ignore"):
            p3 = np.array(intr.img_to_space([pyref.F32(cx), pyref.F32(cy)], pyref.F32(img[cy, cx])), dtype=np.float32)
        for t, leaf in enumerate(leaf_idx[wi]):
            lv = tables.votes(int(leaf))
            if lv is not None:
                yield int(wi), t, int(leaf), p3, lv[0], lv[1]


def frame_votes(tables: LeafTables, model, img, K, leaf_idx, patch_flags):
    """All position votes of one frame: (window index [k], tree [k], cell int64 [k, 3], value [k])."""
    wins, trees, cells, vals = [], [], [], []
    for wi, t, _, p3, v, offs in _voting_hits(tables, model, img, K, leaf_idx, patch_flags):
        with np.errstate(over="ignore", invalid="ignore"):
            d = p3[None, :] - offs                              # f32, prediction.rs:647
        keep = ~(d[:, 2] < 0.0)                                  # :650 (NaN z is kept, as in the reference)
        c = as_i32_vec(d[keep])
        wins.append(np.full(len(c), wi, dtype=np.int64))
        trees.append(np.full(len(c), t, dtype=np.int64))
        cells.append(c)
        vals.append(np.full(len(c), v, dtype=np.uint64))
    if not cells:
        e = np.zeros(0, dtype=np.int64)
        return e, e, np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.uint64)
    return np.concatenate(wins), np.concatenate(trees), np.concatenate(cells), np.concatenate(vals)


def support_from_votes(votes, mid_point, radius: int, model, w: int, h: int) -> dict:
    """The dh_support record of one frame from its position votes."""
    wins, trees, cells, vals = votes
    nx, _ = model.patch_grid(w, h)
    lw, lh, step = int(model.subimage_width) // 2, int(model.subimage_height) // 2, int(model.stepwidth)
    m = as_i32_vec(np.asarray(mid_point, dtype=np.float32))
    sup = np.all(np.abs(cells - m[None, :]) <= int(radius), axis=1) if len(cells) else np.zeros(0, dtype=bool)
    rec = dict.fromkeys(SUPPORT_FIELDS, 0)
    rec["total_mass"] = int(vals.sum(dtype=np.uint64)) if len(vals) else 0
    if sup.any():
        sw = np.unique(wins[sup])
        cx, cy = lw + (sw % nx) * step, lh + (sw // nx) * step
        rec.update(x=int(cx.min()), y=int(cy.min()), width=int(cx.max() - cx.min() + 1), height=int(cy.max() - cy.min() + 1),
                   windows=int(len(sw)), hits=int(len(np.unique(wins[sup] * 1_000_003 + trees[sup]))),
                   mass=int(vals[sup].sum(dtype=np.uint64)))
    return rec


def replay(tables: LeafTables, model, img, K, leaf_idx, patch_flags, mid_point, radii):
    """The dh_support records (dicts) of one frame at each radius of `radii`, and its votes, from any source of taps."""
    img = np.asarray(img, dtype=np.uint16)
    h, w = img.shape
    votes = frame_votes(tables, model, img, K, leaf_idx, patch_flags)
    return [support_from_votes(votes, mid_point, r, model, w, h) for r in radii], votes


def support_ref(oracle, tables: LeafTables, model, img, K, radius: int, midp_guess=None, rot_guess=None):
    """(oracle result, dh_support record as a dict, the frame's votes) of one frame, replayed from the oracle's taps."""
    img = np.asarray(img, dtype=np.uint16)
    res = oracle.predict(tables.forest, model, img, K, midp_guess, rot_guess, taps=True)
    (rec,), votes = replay(tables, model, img, K, res.leaf_idx, res.patch_flags, res.mid_point, [radius])
    return res, rec, votes


def hit_boxes(tables: LeafTables, model, img, K, leaf_idx, patch_flags):
    """HitBox of every hit record with position votes (k_emit.hip): lo, hi int64 [k, 3] = as_i32(p3 - omax), as_i32(p3 - omin),
    differences in f32, the box of a leaf with a non-finite offset unbounded (LeafTables.box)."""
    lo, hi = [], []
    for _, _, leaf, p3, _, _ in _voting_hits(tables, model, img, K, leaf_idx, patch_flags):
        omin, omax = tables.box(leaf)
        with np.errstate(over="ignore", invalid="ignore"):
            lo.append(as_i32_vec(p3 - omax))
            hi.append(as_i32_vec(p3 - omin))
    if not lo:
        return np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)
    return np.stack(lo), np.stack(hi)


BRANCHES = ("skip", "walk_miss", "meets")


def branches(boxes, mid_point, radius: int) -> dict:
    """Hits per case of k_support: the box misses the cube m +- r with lo.z >= 1 (counted without a read), misses with
    lo.z < 1 (offsets walked for total_mass), meets the cube (offsets walked for both sums)."""
    lo, hi = boxes
    m = as_i32_vec(np.asarray(mid_point, dtype=np.float32))
    meets = np.all(lo <= m + int(radius), axis=1) & np.all(hi >= m - int(radius), axis=1)
    return {"skip": int(np.sum(~meets & (lo[:, 2] >= 1))), "walk_miss": int(np.sum(~meets & (lo[:, 2] < 1))),
            "meets": int(np.sum(meets))}


def as_record(rec: dict, dtype) -> np.ndarray:
    out = np.zeros(1, dtype=dtype)
    for k in SUPPORT_FIELDS:
        out[k] = rec[k]
    return out[0]


def densest_cell(oracle, forest, model, img, K):
    """The oracle's heaviest midpoint-accumulator cell of a frame as an f32 midpoint guess (the mean shift then starts on the
    votes and moves), or None for a frame without votes."""
    res = oracle.predict(forest, model, np.asarray(img, dtype=np.uint16), K, taps=True)
    if len(res.mid_cells) == 0:
        return None
    return res.mid_cells[int(np.argmax(res.mid_cells[:, 3].view(np.uint32)))][:3].astype(np.float32)


def head_guesses(oracle, forest, model, frames, Ks):
    """Midpoint guesses [n, 3] f32 and guess mask [n] u8 (bit0 where the frame has votes) from `densest_cell`."""
    n = frames.shape[0]
    mg = np.zeros((n, 3), dtype=np.float32)
    mask = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        g = densest_cell(oracle, forest, model, frames[i], Ks[i] if np.ndim(Ks) == 3 else Ks)
        if g is not None:
            mg[i], mask[i] = g, 1
    return mg, mask


def partial(recs) -> int:
    """Records whose cube holds some but not all of the frame's votes, from more than one window."""
    return int(np.sum((recs["mass"] > 0) & (recs["mass"] < recs["total_mass"]) & (recs["windows"] > 1)))
