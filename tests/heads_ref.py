"""CPU restatement of several heads per frame (include/depthhead_hip.h: dh_head).

TEST INFRASTRUCTURE ONLY.  It starts from the taps of one frame (leaf_idx, patch_flags: the C oracle's or pyref's) and the
forest's leaf tables, replays every position vote with its 20 x 20 guess-grid cell (pyref's f32 projection and clamp,
prediction.rs:647-676) and every rotation vote of the hits that cast position votes (:601-636), and then follows the
definition step by step with Python integers and pyref's f32 / f64 rules:

  seed cells (count descending, index ascending; Chebyshev suppression) -> floor of each seed cell's vote centroid ->
  position mean shift over the whole accumulator -> support record (support_ref) -> rotation from the supporting hits'
  rotation votes only -> drop mass 0, merge within DH_MEANSHIFT_KERNEL_SIZE, order by mass.

`meanshift` is pyref.meanshift over the non-zero cells of the window only, in the same x -> y -> z order, stopping at a fixed
point (every later iteration repeats it); tests/test_heads_ref.py holds it to pyref.meanshift.
"""
from __future__ import annotations

import numpy as np

from oracle import pyref

import support_ref as sr

MAX_HEADS = 4
HEADS_SUPPRESS = 2
MERGE = 20            # DH_MEANSHIFT_KERNEL_SIZE
F32, F64 = pyref.F32, pyref.F64

_KERNELS = {}


def kernel_array(sigma) -> np.ndarray:
    """pyref.build_kernel(20, sigma) as a [20, 20, 20] f32 array indexed [x][y][z]."""
    key = float(np.float32(sigma))
    if key not in _KERNELS:
        k = pyref.build_kernel(20, F32(sigma))
        a = np.zeros((20, 20, 20), np.float32)
        for (x, y, z), v in k.items():
            a[x, y, z] = v
        _KERNELS[key] = a
    return _KERNELS[key]


def _wrap(a):
    return ((np.asarray(a, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def meanshift(cells: np.ndarray, vals: np.ndarray, init, kern: np.ndarray, iterations: int):
    """pyref.meanshift over an accumulator given as distinct cells [k, 3] int64 with non-zero u32 values [k]."""
    pos = [int(init[0]), int(init[1]), int(init[2])]
    for _ in range(iterations):
        d = _wrap(cells - np.array(pos, np.int64)[None, :]) if len(cells) else np.zeros((0, 3), np.int64)
        sel = np.all((d >= -10) & (d <= 9), axis=1)
        dd, vv = d[sel], vals[sel]
        order = np.lexsort((dd[:, 2], dd[:, 1], dd[:, 0]))
        num = [F32(0.0), F32(0.0), F32(0.0)]
        den = F32(0.0)
        for j in order:
            ap = [pyref.wrap_i32(pos[k] + int(dd[j, k])) for k in range(3)]
            w = F32(kern[dd[j, 0] + 10, dd[j, 1] + 10, dd[j, 2] + 10] * F32(int(vv[j])))
            for k in range(3):
                num[k] = F32(num[k] + F32(F32(ap[k]) * w))
            den = F32(den + w)
        if den == 0.0:
            break
        with np.errstate(divide="ignore", invalid="ignore"):
            new = [pyref.as_i32(F32(num[k] / den)) for k in range(3)]
        if new == pos:
            break
        pos = new
    return tuple(pos)


def _rot_cells(forest, leaf: int):
    """Fine rotation cells [k, 3] of a leaf that passes the rotation gate (prediction.rs:600-627), else None."""
    rots = forest.rotations[forest.rot_begin[leaf]:forest.rot_begin[leaf + 1]]
    if not pyref.trace_of_cov(rots, F64) <= pyref.MAX_VARIANCE_ROT:
        return None
    out = []
    for rv in rots:
        r = []
        for k in range(3):
            b = pyref.wrap_i32(pyref.as_i32(F64(F64(F64(rv[k]) * F64(120)) / F64(360.0))) + 60)
            if b >= 120:
                b -= 120
            elif b < 0:
                b += 120
            r.append(b)
        out.append(r)
    return np.array(out, np.int64).reshape(-1, 3)


def guess_cells(d: np.ndarray, K, w: int, h: int) -> np.ndarray:
    """Guess-grid index of every vote d = p3 - o [k, 3] f32 (prediction.rs:660-676), vectorised in f32."""
    m = np.asarray(K, np.float32).reshape(3, 3)
    with np.errstate(all="ignore"):
        r = [((m[i, 0] * d[:, 0]) + (m[i, 1] * d[:, 1])) + (m[i, 2] * d[:, 2]) for i in range(3)]
        qx, qy = r[0] / r[2], r[1] / r[2]
    x2 = np.where(qx > np.float32(0.0), qx, np.float32(0.0))
    x2 = np.where(x2 < np.float32(w - 1), x2, np.float32(w - 1))
    y2 = np.where(qy > np.float32(0.0), qy, np.float32(0.0))
    y2 = np.where(y2 < np.float32(h - 1), y2, np.float32(h - 1))
    gx = x2.astype(np.int64) * 20 // w
    gy = y2.astype(np.int64) * 20 // h
    return gy * 20 + gx


def frame_hits(tables: sr.LeafTables, model, img, K, leaf_idx, patch_flags):
    """Position votes with guess cells and the rotation votes of their hits: dict of arrays (one row per vote / rot vote)."""
    img = np.asarray(img, np.uint16)
    h, w = img.shape
    wins, trees, cells, vals, gcell, vhit = [], [], [], [], [], []
    rc, rv, rhit = [], [], []
    for hi, (wi, t, leaf, p3, v, offs) in enumerate(sr._voting_hits(tables, model, img, K, leaf_idx, patch_flags)):
        with np.errstate(over="ignore", invalid="ignore"):
            d = p3[None, :] - offs
        keep = ~(d[:, 2] < 0.0)
        d = d[keep]
        c = sr.as_i32_vec(d)
        wins.append(np.full(len(c), wi, np.int64)); trees.append(np.full(len(c), t, np.int64))
        cells.append(c); vals.append(np.full(len(c), v, np.int64)); gcell.append(guess_cells(d, K, w, h))
        vhit.append(np.full(len(c), hi, np.int64))
        rot = tables.__dict__.setdefault("_rot", {})         # per leaf, like LeafTables' own tables
        if leaf not in rot:
            rot[leaf] = _rot_cells(tables.forest, leaf)
        r = rot[leaf]
        if r is not None:
            rc.append(r); rv.append(np.full(len(r), v, np.int64)); rhit.append(np.full(len(r), hi, np.int64))
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape, np.int64)   # noqa: E731
    return dict(wins=cat(wins, 0), trees=cat(trees, 0), cells=cat(cells, (0, 3)), vals=cat(vals, 0), g=cat(gcell, 0),
                hit=cat(vhit, 0), rot_cells=cat(rc, (0, 3)), rot_vals=cat(rv, 0), rot_hit=cat(rhit, 0))


def pos_grid(fh) -> np.ndarray:
    g = np.zeros(400, np.int64)
    np.add.at(g, fh["g"], fh["vals"])
    return g % (1 << 32)


def seed_cells(grid, max_heads: int):
    order = sorted(range(400), key=lambda i: (-int(grid[i]), i))
    picks = []
    for i in order:
        if len(picks) == max_heads or grid[i] == 0:
            break
        if all(max(abs(i % 20 - p % 20), abs(i // 20 - p // 20)) > HEADS_SUPPRESS for p in picks):
            picks.append(i)
    return picks


def exact_sum(vals: np.ndarray, coord: np.ndarray) -> int:
    """sum v * c as a Python integer (c split into 2^20 digits so that no int64 partial sum can overflow)."""
    c = np.asarray(coord, np.int64)
    hi, lo = c >> 20, c & ((1 << 20) - 1)
    return (int(np.sum(vals * hi, dtype=np.int64)) << 20) + int(np.sum(vals * lo, dtype=np.int64))


def seed_point(fh, cell: int):
    sel = fh["g"] == cell
    v = fh["vals"][sel]
    sv = int(v.sum())
    return tuple(exact_sum(v, fh["cells"][sel, k]) // sv for k in range(3))


def accumulate(cells: np.ndarray, vals: np.ndarray):
    """Distinct cells and their u32 sums, zero sums dropped (the reference's HashMap reads 0 there)."""
    if len(cells) == 0:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    u, inv = np.unique(cells, axis=0, return_inverse=True)
    s = np.zeros(len(u), np.int64)
    np.add.at(s, inv.reshape(-1), vals)
    s %= 1 << 32
    nz = s != 0
    return u[nz], s[nz]


def rotation_of(rot_cells, rot_vals, kern, iterations: int):
    """The plain call's rotation rule on a rotation accumulator given as votes: (radians [3] f64, start cell)."""
    grid = np.zeros(8000, np.int64)
    if len(rot_cells):
        rough = rot_cells * 20 // 120
        np.add.at(grid, rough[:, 2] * 400 + rough[:, 1] * 20 + rough[:, 0], rot_vals)
    grid %= 1 << 32
    best = int(np.argmax(grid)) if grid.max() > 0 else 0
    rb = (best % 20, (best // 20) % 20, best // 400)
    deg = [F64(F64(F64(F64(b) * F64(360.0)) + F64(180.0)) / F64(20)) for b in rb]
    start = tuple(pyref.as_i32(F64(F64(g * F64(120)) / F64(360.0))) for g in deg)
    c, v = accumulate(rot_cells, rot_vals)
    res = meanshift(c, v, start, kern, iterations)
    return np.array([F64(F64(F64(F64(r) - F64(F64(120) / F64(2.0))) / F64(60)) * F64(3.14159)) for r in res]), start


def heads_from_hits(fh, model, w: int, h: int, max_heads: int, radius: int, kern=None):
    """(n_heads, [dict(mid_point, rotation, support, seed, seed_cell)], info) of one frame."""
    kern = kernel_array(model.gaussian_sigma) if kern is None else kern
    its = int(model.meanshift_iterations)
    grid = pos_grid(fh)
    picks = seed_cells(grid, max_heads)
    acc_c, acc_v = accumulate(fh["cells"], fh["vals"])
    votes = (fh["wins"], fh["trees"], fh["cells"], fh["vals"].astype(np.uint64))
    cands = []
    for k, cell in enumerate(picks):
        seed = seed_point(fh, cell)
        mid = meanshift(acc_c, acc_v, seed, kern, its)
        mid_point = np.array([F32(mid[0]), F32(mid[1]), F32(pyref.wrap_i32(mid[2] * pyref.ZSCALEFACTOR))], np.float32)
        rec = sr.support_from_votes(votes, mid_point, radius, model, w, h)
        m = np.array(mid, np.int64)
        inside = np.all(np.abs(fh["cells"] - m[None, :]) <= int(radius), axis=1) if len(fh["cells"]) else np.zeros(0, bool)
        sup_hits = np.unique(fh["hit"][inside])
        rsel = np.isin(fh["rot_hit"], sup_hits)
        rotation, _ = rotation_of(fh["rot_cells"][rsel], fh["rot_vals"][rsel], kern, its)
        cands.append(dict(k=k, seed_cell=cell, seed=seed, mid=mid, mid_point=mid_point, rotation=rotation, support=rec))
    kept, merged = merge_order(cands)
    return len(kept), kept, dict(picks=picks, grid=grid, merged=merged, candidates=cands)


def merge_order(cands):
    """Step 7 on candidates in seed order (dicts with k, mid, support): (survivors by mass, number merged away)."""
    kept, merged = [], 0
    for c in cands:
        if c["support"]["mass"] == 0:
            continue
        if any(max(abs(c["mid"][q] - o["mid"][q]) for q in range(3)) <= MERGE for o in kept):
            merged += 1
            continue
        kept.append(c)
    kept.sort(key=lambda c: (-c["support"]["mass"], c["k"]))
    return kept, merged


def heads_ref(oracle, tables: sr.LeafTables, model, img, K, max_heads: int = MAX_HEADS, radius: int = 30):
    """heads_from_hits on the C oracle's taps of one frame; also returns the oracle result (its pos_grid is the check)."""
    img = np.asarray(img, np.uint16)
    res = oracle.predict(tables.forest, model, img, K, taps=True)
    fh = frame_hits(tables, model, img, K, res.leaf_idx, res.patch_flags)
    h, w = img.shape
    n, kept, info = heads_from_hits(fh, model, w, h, max_heads, radius)
    assert np.array_equal(info["grid"], res.pos_grid.astype(np.int64)), "guess cells disagree with the oracle's pos_grid"
    return n, kept, info, res, fh


def as_records(n: int, kept, max_heads: int, dtype) -> np.ndarray:
    out = np.zeros(max_heads, dtype=dtype)
    for j, c in enumerate(kept[:max_heads]):
        out[j]["pose"]["mid_point"] = c["mid_point"]
        out[j]["pose"]["rotation"] = c["rotation"]
        for f in sr.SUPPORT_FIELDS:
            out[j]["support"][f] = c["support"][f]
    return out


def composite(depth_a, depth_b):
    """Two depth frames as one scene: each pixel takes the nearer non-zero depth."""
    a, b = np.asarray(depth_a, np.uint16), np.asarray(depth_b, np.uint16)
    both = (a > 0) & (b > 0)
    return np.where(both, np.minimum(a, b), np.maximum(a, b)).astype(np.uint16)
