"""A pure-Python restatement of a multi-head tracker step (include/depthhead_hip.h, "several heads per camera with persistent
identities"), written from the definition and independent of depthhead_amd/csrc/dh_track_heads.h.

Tracks are TRACK_DTYPE records [MAX_TRACKS], heads HEAD_DTYPE records [max_heads]; `step` returns new arrays and leaves its
inputs alone."""
import math

import numpy as np

MAX_TRACKS = 8
U32 = 0xFFFFFFFF


def cell(v) -> int:
    """Rust `f32 as i32`: truncation toward zero, NaN -> 0, saturating."""
    v = float(np.float32(v))
    if math.isnan(v):
        return 0
    if v >= 2147483648.0:
        return 2147483647
    if v <= -2147483648.0:
        return -2147483648
    return int(v)


def cells(mid) -> tuple:
    return tuple(cell(mid[q]) for q in range(3))


def chebyshev(a, b) -> int:
    return max(abs(x - y) for x, y in zip(a, b))


def sat_inc(v) -> int:
    return min(int(v) + 1, U32)


def step(tracks, next_id, heads, n, gate, max_misses, present=True):
    """One camera's step -> (tracks after, next_id after, ids [len(heads)] u32, info) where info counts
    matched / born / coasting / freed / refused heads and tracks."""
    tracks = tracks.copy()
    max_heads = len(heads)
    ids = np.zeros(max_heads, dtype=np.uint32)
    info = dict(matched=0, born=0, coasting=0, freed=0, refused=0)
    if not present:
        return tracks, next_id, ids, info
    n = min(int(n), max_heads)
    live = [t for t in range(MAX_TRACKS) if tracks[t]["id"] != 0]
    tc = {t: cells(tracks[t]["head"]["pose"]["mid_point"]) for t in live}
    hc = [cells(heads[j]["pose"]["mid_point"]) for j in range(n)]
    pairs = sorted((chebyshev(tc[t], hc[j]), j, t) for j in range(n) for t in live)
    used_t, used_h = set(), set()
    for d, j, t in pairs:
        if d > gate or t in used_t or j in used_h:
            continue
        used_t.add(t)
        used_h.add(j)
        tracks[t]["head"] = heads[j]
        tracks[t]["hits"] = sat_inc(tracks[t]["hits"])
        tracks[t]["age"] = sat_inc(tracks[t]["age"])
        tracks[t]["misses"] = 0
        ids[j] = tracks[t]["id"]
        info["matched"] += 1
    for t in live:
        if t in used_t:
            continue
        tracks[t]["age"] = sat_inc(tracks[t]["age"])
        tracks[t]["misses"] = sat_inc(tracks[t]["misses"])
        info["coasting"] += 1
        if int(tracks[t]["misses"]) > max_misses:
            tracks[t] = np.zeros((), dtype=tracks.dtype)
            info["freed"] += 1
    for j in range(n):
        if j in used_h:
            continue
        free = [t for t in range(MAX_TRACKS) if tracks[t]["id"] == 0]
        if not free:
            info["refused"] += 1
            continue
        t = free[0]
        tracks[t] = np.zeros((), dtype=tracks.dtype)
        tracks[t]["id"] = next_id
        tracks[t]["age"] = 1
        tracks[t]["hits"] = 1
        tracks[t]["head"] = heads[j]
        ids[j] = next_id
        next_id = 1 if next_id == U32 else next_id + 1
        info["born"] += 1
    return tracks, next_id, ids, info


class Restatement:
    """Every camera of a tracker: fed the heads of each step, it keeps the state the GPU should hold."""

    def __init__(self, n_cams, max_heads, gate, max_misses, track_dtype):
        self.n, self.max_heads, self.gate, self.max_misses = n_cams, max_heads, gate, max_misses
        self.tracks = np.zeros((n_cams, MAX_TRACKS), dtype=track_dtype)
        self.next_id = np.ones(n_cams, dtype=np.uint32)
        self.totals = dict(matched=0, born=0, coasting=0, freed=0, refused=0)

    def reset(self, camera=None):
        cams = range(self.n) if camera is None else [camera]
        for c in cams:
            self.tracks[c] = np.zeros(MAX_TRACKS, dtype=self.tracks.dtype)
            self.next_id[c] = 1

    def step(self, n_heads, heads, present=None):
        ids = np.zeros((self.n, self.max_heads), dtype=np.uint32)
        for c in range(self.n):
            pres = present is None or present[c] != 0
            tr, nid, ids[c], info = step(self.tracks[c], int(self.next_id[c]), heads[c], n_heads[c], self.gate,
                                         self.max_misses, pres)
            self.tracks[c], self.next_id[c] = tr, nid
            for k, v in info.items():
                self.totals[k] += v
        return ids, self.tracks.copy()
