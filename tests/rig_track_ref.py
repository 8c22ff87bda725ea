"""A pure-Python restatement of a rig tracker step (include/depthhead_hip.h, "camera rigs"), written from
the definition in the header and independent of depthhead_amd/csrc/dh_rig.h: numpy float32 scalars for the world transform,
Python integers for everything else.

Tracks are RIG_TRACK_DTYPE records [MAX_TRACKS], persons RIG_PERSON_DTYPE records [MAX_PERSONS], heads HEAD_DTYPE records
[n_cams][max_heads]; `step` returns new arrays and leaves its inputs alone."""
import math

import numpy as np

MAX_CAMERAS = 64
MAX_PERSONS = 16
MAX_TRACKS = 16
U32 = 0xFFFFFFFF
U64 = 0xFFFFFFFFFFFFFFFF


def cell(v) -> int:
    """(int32_t) of an f32 as the support calls convert: truncation toward zero, NaN -> 0, saturating."""
    v = float(np.float32(v))
    if math.isnan(v):
        return 0
    if v >= 2147483648.0:
        return 2147483647
    if v <= -2147483648.0:
        return -2147483648
    return int(v)


def world(R, t, m):
    """((R[q][0] m0 + R[q][1] m1) + R[q][2] m2) + t[q] in f32, every operation rounded on its own -> np.float32 [3]"""
    R = np.asarray(R, dtype=np.float32).reshape(3, 3)
    t = np.asarray(t, dtype=np.float32).reshape(3)
    m = np.asarray(m, dtype=np.float32).reshape(3)
    out = np.zeros(3, dtype=np.float32)
    with np.errstate(all="ignore"):
        for q in range(3):
            a = np.float32(R[q, 0] * m[0])
            b = np.float32(R[q, 1] * m[1])
            c = np.float32(R[q, 2] * m[2])
            out[q] = np.float32(np.float32(np.float32(a + b) + c) + t[q])
    return out


def chebyshev(a, b) -> int:
    return max(abs(int(x) - int(y)) for x, y in zip(a, b))


def sat_inc(v) -> int:
    return min(int(v) + 1, U32)


def step(tracks, next_id, R, t, present, n_heads, heads, cam0, fuse_gate, gate, max_misses, person_dtype):
    """One rig's step.  R [n_cams, 9], t [n_cams, 3], present None or [n_cams], n_heads [n_cams], heads [n_cams, max_heads];
    cam0: the table index of the rig's first camera.
    -> (tracks after, next_id after, ids u32 [n_cams, max_heads], n_persons, persons [MAX_PERSONS], info)"""
    tracks = tracks.copy()
    n_cams, max_heads = heads.shape
    ids = np.zeros((n_cams, max_heads), dtype=np.uint32)
    persons = np.zeros(MAX_PERSONS, dtype=person_dtype)
    info = dict(matched=0, born=0, coasting=0, freed=0, refused=0, unassigned=0, multi_view=0, single_view=0)
    pres = [present is None or present[k] != 0 for k in range(n_cams)]
    if not any(pres):
        return tracks, next_id, ids, 0, persons, info
    # the heads of the present cameras, their world midpoints and cells
    hs = []
    for k in range(n_cams):
        if not pres[k]:
            continue
        for j in range(min(int(n_heads[k]), max_heads)):
            w = world(R[k], t[k], heads[k, j]["pose"]["mid_point"])
            hs.append(dict(k=k, j=j, world=w, cell=tuple(cell(x) for x in w), mass=int(heads[k, j]["support"]["mass"])))
    hs.sort(key=lambda h: (-h["mass"], h["k"], h["j"]))
    # fuse
    ps = []
    for h in hs:
        for p in ps:
            if chebyshev(p["anchor"]["cell"], h["cell"]) <= fuse_gate and all(m["k"] != h["k"] for m in p["members"]):
                p["members"].append(h)
                h["person"] = p
                break
        else:
            if len(ps) < MAX_PERSONS:
                p = dict(anchor=h, members=[h])
                ps.append(p)
                h["person"] = p
            else:
                h["person"] = None
                info["unassigned"] += 1
    # person records
    for i, p in enumerate(ps):
        rec = persons[i]
        nm = len(p["members"])
        rec["cell"] = [sum(m["cell"][q] for m in p["members"]) // nm for q in range(3)]     # Python's // floors
        rec["views"] = sum(1 << m["k"] for m in p["members"])
        rec["n_views"] = nm
        rec["mass"] = min(sum(m["mass"] for m in p["members"]), U64)
        rec["best_cam"] = cam0 + p["anchor"]["k"]
        rec["best_head"] = p["anchor"]["j"]
        rec["world"] = p["anchor"]["world"]
        info["multi_view" if nm > 1 else "single_view"] += 1
    # match
    live = [s for s in range(MAX_TRACKS) if tracks[s]["id"] != 0]
    pairs = sorted((chebyshev(tracks[s]["person"]["cell"], persons[i]["cell"]), i, s) for i in range(len(ps)) for s in live)
    used_t, used_p = set(), set()
    for d, i, s in pairs:
        if d > gate or s in used_t or i in used_p:
            continue
        used_t.add(s)
        used_p.add(i)
        persons[i]["id"] = tracks[s]["id"]
        tracks[s]["person"] = persons[i]
        tracks[s]["hits"] = sat_inc(tracks[s]["hits"])
        tracks[s]["age"] = sat_inc(tracks[s]["age"])
        tracks[s]["misses"] = 0
        info["matched"] += 1
    for s in live:
        if s in used_t:
            continue
        tracks[s]["age"] = sat_inc(tracks[s]["age"])
        tracks[s]["misses"] = sat_inc(tracks[s]["misses"])
        info["coasting"] += 1
        if int(tracks[s]["misses"]) > max_misses:
            tracks[s] = np.zeros((), dtype=tracks.dtype)
            info["freed"] += 1
    for i in range(len(ps)):
        if i in used_p:
            continue
        free = [s for s in range(MAX_TRACKS) if tracks[s]["id"] == 0]
        if not free:
            info["refused"] += 1
            continue
        s = free[0]
        persons[i]["id"] = next_id
        tracks[s] = np.zeros((), dtype=tracks.dtype)
        tracks[s]["id"] = next_id
        tracks[s]["age"] = 1
        tracks[s]["hits"] = 1
        tracks[s]["person"] = persons[i]
        next_id = 1 if next_id == U32 else next_id + 1
        info["born"] += 1
    for h in hs:
        if h["person"] is not None:
            ids[h["k"], h["j"]] = persons[ps.index(h["person"])]["id"]
    return tracks, next_id, ids, len(ps), persons, info


class Restatement:
    """Every rig of a tracker: fed the heads of each step, it keeps the state the GPU should hold."""

    def __init__(self, R, t, rig_begin, max_heads, fuse_gate, gate, max_misses, track_dtype, person_dtype):
        self.R = np.asarray(R, dtype=np.float32).reshape(-1, 9)
        self.t = np.asarray(t, dtype=np.float32).reshape(-1, 3)
        self.rig_begin = [int(x) for x in rig_begin]
        self.n_rigs = len(self.rig_begin) - 1
        self.n = self.rig_begin[-1]
        self.max_heads, self.fuse_gate, self.gate, self.max_misses = max_heads, fuse_gate, gate, max_misses
        self.person_dtype = person_dtype
        self.tracks = np.zeros((self.n_rigs, MAX_TRACKS), dtype=track_dtype)
        self.next_id = np.ones(self.n_rigs, dtype=np.uint32)
        self.totals = {}

    def reset(self, rig=None):
        for g in range(self.n_rigs) if rig is None else [rig]:
            self.tracks[g] = np.zeros(MAX_TRACKS, dtype=self.tracks.dtype)
            self.next_id[g] = 1

    def step(self, n_heads, heads, present=None):
        """-> (ids [n, max_heads], n_persons [n_rigs], persons [n_rigs, MAX_PERSONS], tracks after [n_rigs, MAX_TRACKS])"""
        ids = np.zeros((self.n, self.max_heads), dtype=np.uint32)
        n_persons = np.zeros(self.n_rigs, dtype=np.uint32)
        persons = np.zeros((self.n_rigs, MAX_PERSONS), dtype=self.person_dtype)
        for g in range(self.n_rigs):
            a, b = self.rig_begin[g], self.rig_begin[g + 1]
            tr, nid, ids[a:b], n_persons[g], persons[g], info = step(
                self.tracks[g], int(self.next_id[g]), self.R[a:b], self.t[a:b], None if present is None else present[a:b],
                n_heads[a:b], heads[a:b], a, self.fuse_gate, self.gate, self.max_misses, self.person_dtype)
            self.tracks[g], self.next_id[g] = tr, nid
            for k, v in info.items():
                self.totals[k] = self.totals.get(k, 0) + v
        return ids, n_persons, persons, self.tracks.copy()
