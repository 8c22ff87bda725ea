"""The rig tracker's step (depthhead_amd/csrc/dh_rig.h, the header k_rig_fuse is built from) against the restatement of
tests/rig_track_ref.py, step by step over hand-built and random sequences.  Fusion: the fuse gate's boundary (gates 100, 0, 7),
two heads of one camera, the order that decides between two anchors (mass, camera, head), the floor of a negative mean, a 17th
person, mass saturation.  Matching, as tests/test_multi_track_rule.py holds section 15: the gate's boundary, both tie orders,
coasting and expiry (max_misses 3, 1, 0), a 17th track refused, the lowest freed slot reused, next_id wrapping.  NaN / inf /
saturating midpoints, extrinsics that overflow f32, rigs of 1 and of 64 cameras, a rig without a present camera.  A one-camera
rig with R = I, t = 0 gives every head the id tests/multi_track_ref.py gives it.  The header is compiled by plain g++
(tests/host/rig_check.cpp), and again under ASan / UBSan."""
import os
import sys

import numpy as np
import pytest

from depthhead_amd._lib import HEAD_DTYPE, RIG_PERSON_DTYPE, RIG_TRACK_DTYPE, TRACK_DTYPE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_program as hp  # noqa: E402
import multi_track_ref as mr  # noqa: E402
import rig_track_ref as rr  # noqa: E402

U32, U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
INF, NAN = float("inf"), float("nan")
EYE = np.eye(3, dtype=np.float32).reshape(9)
Z = 1000.5


def head(mid, mass, tag=0):
    """A HEAD_DTYPE record at midpoint `mid` with support mass `mass`; the other fields carry `tag`."""
    h = np.zeros((), dtype=HEAD_DTYPE)
    h["pose"]["mid_point"] = np.asarray(mid, dtype=np.float32)
    h["pose"]["rotation"] = (0.5 * tag, -0.25 * tag, tag + 0.125)
    s = h["support"]
    s["x"], s["y"], s["width"], s["height"] = tag, tag + 1, tag + 2, tag + 3
    s["windows"], s["hits"], s["mass"], s["total_mass"] = tag + 4, tag + 5, mass, U64
    return h


class Seq:
    """One rig's sequence.  A step is (per camera a list of (mid, mass), present or None, n_heads override or None)."""

    def __init__(self, name, n_cams=1, max_heads=4, fuse_gate=100, gate=100, max_misses=3, R=None, t=None, cam0=0, tracks=None,
                 next_id=1):
        self.name, self.n_cams, self.max_heads = name, n_cams, max_heads
        self.fuse_gate, self.gate, self.max_misses, self.cam0 = fuse_gate, gate, max_misses, cam0
        self.R = np.tile(EYE, (n_cams, 1)) if R is None else np.asarray(R, dtype=np.float32).reshape(n_cams, 9)
        self.t = np.zeros((n_cams, 3), dtype=np.float32) if t is None else np.asarray(t, dtype=np.float32).reshape(n_cams, 3)
        self.tracks = np.zeros(rr.MAX_TRACKS, dtype=RIG_TRACK_DTYPE) if tracks is None else tracks
        self.next_id = next_id
        self.steps = []

    def add(self, cams, present=None, n=None):
        hs = np.zeros((self.n_cams, self.max_heads), dtype=HEAD_DTYPE)
        nh = np.zeros(self.n_cams, dtype=np.uint32)
        for k, lst in enumerate(cams):
            for j, (mid, mass) in enumerate(lst):
                hs[k, j] = head(mid, mass, tag=100 * len(self.steps) + 4 * k + j + 1)
            nh[k] = len(lst)
        if n is not None:
            nh[:] = n
        self.steps.append((hs, nh, None if present is None else np.asarray(present, dtype=np.uint8)))
        return self


def hand_sequences():
    seqs = []
    # the fuse gate: d == fuse_gate is one person, fuse_gate + 1 two (also through t, and along z)
    for g in (100, 0, 7):
        seqs.append(Seq(f"fuse {g}", 2, fuse_gate=g).add([[((0.5, 0, Z), 10)], [((g + 0.5, 0, Z), 5)]])
                    .add([[((0.5, 0, Z), 10)], [((g + 1.5, 0, Z), 5)]]))
        seqs.append(Seq(f"fuse {g} t", 2, fuse_gate=g, t=[(0, 0, 0), (0, 0, -g)]).add([[((0, 0, Z), 10)], [((0, 0, Z), 5)]])
                    .add([[((0, 0, Z), 10)], [((0, 0, Z - 1), 5)]]))
    # two heads of one camera within the gate stay two persons; the other camera's head joins the first of them
    seqs.append(Seq("one camera", 2).add([[((0, 0, Z), 10), ((30, 0, Z), 9)], [((15, 0, Z), 5)]]))
    # a head within the gate of two anchors joins the one created first: mass decides, then the camera, then the head index
    a, b, c = (0, 0, Z), (150, 0, Z), (75, 0, Z)
    seqs.append(Seq("order mass", 3).add([[(a, 10)], [(b, 9)], [(c, 5)]]).add([[(a, 9)], [(b, 10)], [(c, 5)]]))
    seqs.append(Seq("order camera", 3).add([[(a, 7)], [(b, 7)], [(c, 7)]]).add([[(b, 7)], [(a, 7)], [(c, 7)]]))
    seqs.append(Seq("order head", 2).add([[(a, 7), (b, 7)], [(c, 7)]]).add([[(b, 7), (a, 7)], [(c, 7)]]))
    # the mean cell is floored toward minus infinity: cells -3 and 0 -> -2; -7, -2, 0 -> -3
    seqs.append(Seq("floor", 3).add([[((-3.5, -7.2, Z), 9)], [((0.5, -2.9, Z), 8)], []]).add([[((-3.5, -7.2, Z), 9)], [((0.5, -2.9, Z), 8)], [((-1, 0.9, Z), 1)]]))
    # a 17th person stays unassigned; then 16 tracks are full and every new person is refused (id 0)
    far = [[((1000 * (4 * k + j), 0, Z), 100 - 4 * k - j) for j in range(4)] for k in range(5)]
    far2 = [[((1000 * (4 * k + j), 5000, Z), 100 - 4 * k - j) for j in range(4)] for k in range(5)]
    seqs.append(Seq("17th", 5, fuse_gate=0, gate=0, max_misses=2).add(far).add(far2).add(far2).add(far2).add(far2))
    # mass saturates at UINT64_MAX
    seqs.append(Seq("mass", 3).add([[(a, 1 << 63)], [(a, 1 << 63)], [(a, 5)]]).add([[(a, U64)], [(a, 1)], []]))
    # ---- the match, as section 15's list
    for g in (100, 0, 7):
        seqs.append(Seq(f"gate {g}", gate=g).add([[((0.9, 0, Z), 5)]]).add([[((g + 0.9, 0, Z), 5)]]).add([[((2 * g + 1.9, -0.5, Z), 5)]]))
    seqs.append(Seq("tie persons", fuse_gate=0).add([[((0, 0, Z), 5)]]).add([[((30, 0, Z), 5), ((-30, 0, Z), 5)]])
                .add([[((-30, 0, Z), 5), ((30, 0, Z), 5)]]))
    seqs.append(Seq("tie tracks", fuse_gate=0).add([[((-40, 0, Z), 5), ((40, 0, Z), 5)]]).add([[((0, 0, Z), 5)]])
                .add([[((0, 0, Z), 5), ((80, 0, Z), 5)]]))
    for mm in (3, 0, 1):
        s = Seq(f"expiry {mm}", max_misses=mm).add([[((0, 0, Z), 9), ((300, 0, Z), 8)]])
        for _ in range(mm + 1):
            s.add([[((300, 0, Z), 8)]])
        s.add([[((0, 0, Z), 9), ((300, 0, Z), 8)]])
        seqs.append(s)
    s = Seq("reuse", gate=0, max_misses=0)
    s.add([[((0, 0, Z), 9), ((1000, 0, Z), 8), ((2000, 0, Z), 7), ((3000, 0, Z), 6)]])
    s.add([[((0, 0, Z), 9), ((3000, 0, Z), 6)]])                       # slots 1 and 2 freed
    s.add([[((0, 0, Z), 9), ((3000, 0, Z), 6), ((5000, 0, Z), 5)]])    # born in slot 1
    seqs.append(s)
    seqs.append(Seq("wrap", gate=0, next_id=U32 - 1).add([[((0, 0, Z), 9), ((500, 0, Z), 8), ((900, 0, Z), 7)]])
                .add([[((0, 0, Z), 9), ((0, 500, Z), 8)]]))
    # NaN, +-inf and saturating midpoints; extrinsics that overflow f32 (finite entries, infinite or NaN world midpoints)
    s = Seq("non-finite", 2, fuse_gate=5, gate=5)
    s.add([[((NAN, 0, Z), 9), ((INF, 1e12, Z), 8), ((-INF, -1e12, -3e9), 7)], [((0.5, NAN, Z), 9), ((3e9, 2.2e9, Z), 8)]])
    s.add([[((NAN, NAN, NAN), 9), ((INF, INF, INF), 8), ((2147483520.0, -2147483648.0, 0), 7)], [((-2.2e9, -INF, -INF), 3)]])
    seqs.append(s)
    big = np.array([3e38, 3e38, 0, -3e38, 3e38, 0, 1e30, 0, 1], dtype=np.float32)
    s = Seq("overflow", 2, R=[big, EYE], t=[(3e38, -3e38, 0), (3.4e38, 0, 0)])
    s.add([[((10, 10, Z), 9), ((1, -1, Z), 8), ((1e10, 5, 1e10), 7)], [((3.4e38, 0, Z), 9), ((-3.4e38, 0, Z), 8)]])
    s.add([[((10, 10, Z), 9), ((2, -2, Z), 8)], [((1e38, 0, Z), 9)]])
    seqs.append(s)
    # a rig without a present camera keeps its whole state; one absent camera contributes nothing; n_heads beyond max_heads
    s = Seq("absent", 2, max_heads=2).add([[(a, 9), (b, 8)], [(a, 7)]])
    s.add([[(a, 9)], [(b, 7)]], present=[0, 0]).add([[(a, 9)], [(b, 7)]], present=[0, 0])
    s.add([[(a, 9)], [((500, 0, Z), 7)]], present=[1, 0]).add([[], []]).add([[(a, 9), (b, 8)], [(a, 7), (b, 6)]], n=7)
    seqs.append(s)
    # a rig whose first camera is camera 37 of the table: best_cam is the table index, views are relative
    seqs.append(Seq("cam0", 3, cam0=37).add([[(a, 5)], [(b, 9)], [(a, 6), (b, 1)]]))
    # saturating counters
    tr = np.zeros(rr.MAX_TRACKS, dtype=RIG_TRACK_DTYPE)
    tr[0]["id"], tr[0]["age"], tr[0]["hits"] = 5, U32 - 1, U32 - 1
    tr[0]["person"]["cell"] = (0, 0, 1000)
    tr[9]["id"], tr[9]["age"], tr[9]["hits"], tr[9]["misses"] = 9, U32, 17, U32 - 1
    tr[9]["person"]["cell"] = (5000, 0, 1000)
    seqs.append(Seq("saturation", max_misses=U32, tracks=tr, next_id=10).add([[(a, 5)]]).add([[(a, 5)]]).add([[(a, 5)]]))
    return seqs


PERMS = [np.eye(3), np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]]), np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]]),
         np.array([[-1, 0, 0], [0, 0, 1], [0, 1, 0]])]


def random_sequences(count=64, seed=17, big=True):
    """People walking in a world frame, each camera (an exact permutation / sign matrix and an integer t, or an arbitrary R)
    seeing some of them with noise of the order of the fuse gate."""
    rs = np.random.RandomState(seed)
    seqs = []
    for i in range(count):
        n_cams = 64 if big and i % 16 == 7 else int(rs.randint(1, 7))
        s = Seq(f"random {i}", n_cams, max_heads=int(rs.randint(1, 5)), fuse_gate=int(rs.choice([0, 30, 100, 100, 2**31 - 1])),
                gate=int(rs.choice([0, 40, 100, 100, 2**31 - 1])), max_misses=int(rs.choice([0, 1, 3, 5, U32])),
                next_id=int(rs.choice([1, 7, U32 - 2])), cam0=int(rs.randint(0, 100)))
        P = [PERMS[rs.randint(len(PERMS))] for _ in range(n_cams)]
        s.t = rs.randint(-2000, 2000, (n_cams, 3)).astype(np.float32)
        s.R = np.stack([p.reshape(9) for p in P]).astype(np.float32)
        if i % 9 == 4:
            s.R = rs.uniform(-1.5, 1.5, (n_cams, 9)).astype(np.float32)     # not orthonormal: the rule only applies R
        n_people = int(rs.randint(1, 22 if i % 5 == 0 else 7))
        pos = rs.uniform(-1500, 1500, (n_people, 3)) + np.array([0, 0, 3000])
        for _ in range(int(rs.randint(4, 12))):
            pos += rs.normal(0, rs.choice([5, 40, 150]), pos.shape)
            cams = []
            for k in range(n_cams):
                seen = rs.permutation(n_people)[: int(rs.randint(0, s.max_heads + 1))]
                lst = []
                for q in seen:
                    w = pos[q] + rs.normal(0, rs.choice([0.1, 20, 60]), 3)
                    lst.append((tuple(P[k].T @ (w - s.t[k])), int(rs.choice([rs.randint(1, 50), 1000, rs.randint(1, 1 << 40)]))))
                cams.append(lst)
            present = None if rs.rand() < 0.5 else (rs.rand(n_cams) > (0.9 if rs.rand() < 0.1 else 0.2)).astype(np.uint8)
            s.add(cams, present)
        seqs.append(s)
    return seqs


def _build(tmp_path, sanitize):
    return hp.build(tmp_path, "rig_check", [hp.host("rig_check.cpp")], sanitize, (*hp.WARN, "-I" + hp.CSRC))


def run_checker(exe, cases):
    """cases: (seq, tracks, next_id, (heads, n_heads, present)) -> [(tracks, next_id, ids, n_persons, persons)]"""
    buf = bytearray()
    for s, tr, nid, (hs, nh, pres) in cases:
        buf += np.array([s.n_cams, s.max_heads, s.fuse_gate, s.gate, s.max_misses, nid, s.cam0, pres is not None], dtype=np.uint32).tobytes()
        buf += np.ascontiguousarray(tr).tobytes() + s.R.tobytes() + s.t.tobytes()
        buf += (np.zeros(s.n_cams, np.uint32) if pres is None else pres.astype(np.uint32)).tobytes()
        buf += nh.tobytes() + np.ascontiguousarray(hs).tobytes()
    run = hp.run(exe, stdin=bytes(buf), timeout=300)
    out, pos, res = run.stdout, 0, []

    def take(dtype, count):
        nonlocal pos
        v = np.frombuffer(out, dtype=dtype, count=count, offset=pos).copy()
        pos += v.nbytes
        return v
    for s, *_ in cases:
        tr = take(RIG_TRACK_DTYPE, rr.MAX_TRACKS)
        nid = int(take(np.uint32, 1)[0])
        ids = take(np.uint32, s.n_cams * s.max_heads).reshape(s.n_cams, s.max_heads)
        npers = int(take(np.uint32, 1)[0])
        res.append((tr, nid, ids, npers, take(RIG_PERSON_DTYPE, rr.MAX_PERSONS)))
    assert pos == len(out)
    return res


def drive(exe, seqs):
    """Every sequence step by step through the header and the restatement; both must agree on every output byte.
    -> per sequence the list of (ids, n_persons, persons, tracks, info) of its steps, and the totals of the info."""
    state = [(s.tracks.copy(), s.next_id) for s in seqs]
    hist = [[] for _ in seqs]
    totals = {}
    for k in range(max(len(s.steps) for s in seqs)):
        live = [i for i, s in enumerate(seqs) if k < len(s.steps)]
        got = run_checker(exe, [(seqs[i], state[i][0], state[i][1], seqs[i].steps[k]) for i in live])
        for i, (tr, nid, ids, npers, persons) in zip(live, got):
            s = seqs[i]
            hs, nh, pres = s.steps[k]
            w_tr, w_nid, w_ids, w_np, w_persons, info = rr.step(state[i][0], state[i][1], s.R, s.t, pres, nh, hs, s.cam0,
                                                                s.fuse_gate, s.gate, s.max_misses, RIG_PERSON_DTYPE)
            assert np.array_equal(ids, w_ids), (s.name, k, ids, w_ids)
            assert npers == w_np, (s.name, k, npers, w_np)
            assert persons.tobytes() == w_persons.tobytes(), (s.name, k, persons, w_persons)
            assert tr.tobytes() == w_tr.tobytes(), (s.name, k, tr, w_tr)
            assert nid == w_nid, (s.name, k, nid, w_nid)
            state[i] = (tr, nid)
            hist[i].append((ids, npers, persons, tr, info))
            for key, v in info.items():
                totals[key] = totals.get(key, 0) + v
    return hist, totals


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("rigc"), None)


def test_hand_cases_match_restatement(checker):
    seqs = hand_sequences()
    hist, totals = drive(checker, seqs)
    h = {s.name: x for s, x in zip(seqs, hist)}
    for g in (100, 0, 7):
        for name in (f"fuse {g}", f"fuse {g} t"):
            assert h[name][0][1] == 1 and h[name][0][2][0]["n_views"] == 2 and h[name][0][2][0]["views"] == 3, name
            assert h[name][1][1] == 2 and list(h[name][1][2]["n_views"][:2]) == [1, 1], name     # fuse_gate + 1: two persons
            assert h[name][0][0][0, 0] == h[name][0][0][1, 0] != 0
    oc = h["one camera"][0]
    assert oc[1] == 2 and list(oc[2]["views"][:2]) == [3, 1] and list(oc[0][:, 0]) == [1, 1] and oc[0][0, 1] == 2
    om = h["order mass"]
    assert list(om[0][2]["views"][:2]) == [5, 2] and list(om[1][2]["views"][:2]) == [6, 1]       # C joins the heavier anchor
    ocam = h["order camera"]
    assert list(ocam[0][2]["views"][:2]) == [5, 2] and list(ocam[0][2]["cell"][0]) == [37, 0, 1000]
    assert list(ocam[1][2]["cell"][0]) == [112, 0, 1000]                                           # equal masses: camera 0 first
    oh = h["order head"]
    assert list(oh[0][2]["cell"][0]) == [37, 0, 1000] and list(oh[1][2]["cell"][0]) == [112, 0, 1000]
    fl = h["floor"]
    assert list(fl[0][2]["cell"][0]) == [-2, -5, 1000] and list(fl[1][2]["cell"][0]) == [-2, -3, 1000], fl[1][2]["cell"][0]
    s17 = h["17th"]
    assert s17[0][1] == 16 and s17[0][4]["unassigned"] == 4 and np.count_nonzero(s17[0][0]) == 16
    assert s17[1][4]["refused"] == 16 and not s17[1][0].any() and s17[1][1] == 16                 # a 17th track is refused
    assert s17[3][4]["freed"] == 16 and np.count_nonzero(s17[3][0]) == 16                          # freed, then born again
    assert h["mass"][0][2]["mass"][0] == U64 and h["mass"][1][2]["mass"][0] == U64
    for g in (100, 0, 7):
        ids = [int(x[0][0, 0]) for x in h[f"gate {g}"]]
        assert ids == [1, 1, 2], (g, ids)
    assert list(h["tie persons"][1][0][0, :2]) == [1, 2] and list(h["tie persons"][2][0][0, :2]) == [2, 1]
    assert list(h["tie tracks"][1][0][0, :1]) == [1]
    for mm in (3, 0, 1):
        e = h[f"expiry {mm}"]
        for k in range(1, mm + 1):
            assert e[k][3][0]["id"] == 1 and e[k][3][0]["misses"] == k and e[k][3][0]["age"] == k + 1, (mm, k)
        assert e[mm + 1][3][0]["id"] == 0 and e[mm + 1][4]["freed"] == 1, mm
        assert list(e[-1][0][0, :2]) == [3, 2] and e[-1][3][0]["id"] == 3
    assert list(h["reuse"][2][3]["id"][:4]) == [1, 5, 0, 4]
    assert list(h["wrap"][0][0][0, :3]) == [U32 - 1, U32, 1] and h["wrap"][1][0][0, 1] == 2
    ab = h["absent"]
    assert ab[1][3].tobytes() == ab[0][3].tobytes() == ab[2][3].tobytes() and ab[1][1] == 0 and not ab[1][0].any()
    assert not ab[3][0][1].any() and ab[3][3][0]["age"] == 2 and ab[4][4]["coasting"] >= 1 and ab[5][1] >= 2
    c0 = h["cam0"][0]
    assert c0[2]["best_cam"][0] == 38 and c0[2]["views"][0] == 6 and c0[2]["best_cam"][1] == 39 and c0[2]["best_head"][1] == 0
    sat = h["saturation"][-1][3]
    assert sat[0]["age"] == U32 and sat[0]["hits"] == U32 and sat[9]["misses"] == U32 and sat[9]["id"] == 9
    ov = h["overflow"][0]
    assert ov[1] >= 2 and {2**31 - 1, -2**31, 0} <= set(int(v) for v in ov[2]["cell"][: ov[1]].reshape(-1))
    for key in ("matched", "born", "coasting", "freed", "refused", "unassigned", "multi_view", "single_view"):
        assert totals[key] >= 1, totals


def test_random_sequences_match_restatement(checker):
    seqs = random_sequences()
    assert len(seqs) >= 60 and sum(s.n_cams == 64 for s in seqs) >= 2 and sum(s.n_cams == 1 for s in seqs) >= 2
    _, totals = drive(checker, seqs)
    for key in ("matched", "born", "coasting", "freed", "refused", "unassigned", "multi_view", "single_view"):
        assert totals[key] >= 5, totals


def test_rule_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "address,undefined")
    drive(exe, hand_sequences() + random_sequences(20, seed=5))


def test_one_camera_rig_gives_the_multi_tracker_ids(checker):
    """Code that already exists: a one-camera rig with R = I, t = 0 never fuses, its persons are its heads in their own order
    (the heads pipeline orders them by mass descending), and the match is section 15's: every head gets the id
    tests/multi_track_ref.py gives it, as long as no more than 8 tracks are live (section 15 has 8 slots, a rig 16)."""
    rs = np.random.RandomState(23)
    seqs, want = [], []
    for i in range(40):
        s = Seq(f"single {i}", 1, max_heads=int(rs.randint(1, 5)), fuse_gate=int(rs.choice([0, 100])), gate=int(rs.choice([0, 40, 100])),
                max_misses=int(rs.choice([0, 1, 3])), next_id=int(rs.choice([1, U32 - 2])))
        pos = rs.uniform(-400, 400, (5, 3)) + np.array([0, 0, 1000])
        tr, nid, ids_seq, ok = np.zeros(mr.MAX_TRACKS, dtype=TRACK_DTYPE), s.next_id, [], True
        for _ in range(int(rs.randint(4, 14))):
            pos += rs.normal(0, rs.choice([5, 40, 150]), pos.shape)
            k = int(rs.randint(0, s.max_heads + 1))
            s.add([[(tuple(pos[q]), 1000 - 10 * j) for j, q in enumerate(rs.permutation(5)[:k])]], present=[int(rs.rand() > 0.15)])
            hs, nh, pres = s.steps[-1]
            tr, nid, ids, info = mr.step(tr, nid, hs[0], nh[0], s.gate, s.max_misses, bool(pres[0]))
            ok = ok and info["refused"] == 0 and np.count_nonzero(tr["id"]) <= 8
            ids_seq.append(ids)
        if ok:
            seqs.append(s)
            want.append(ids_seq)
    assert len(seqs) >= 25, len(seqs)
    hist, _ = drive(checker, seqs)
    for s, hx, wx in zip(seqs, hist, want):
        for k, (x, w) in enumerate(zip(hx, wx)):
            assert np.array_equal(x[0][0], w), (s.name, k, x[0][0], w)


def test_restatement_at_its_edges():
    """The restatement itself: cells of non-finite values, the separately rounded transform, the floored mean."""
    assert [rr.cell(v) for v in (NAN, INF, -INF, 3e9, -3e9, -0.9, 0.9, -2147483648.0)] == \
           [0, 2**31 - 1, -2**31, 2**31 - 1, -2**31, 0, 0, -2**31]
    # 1 + 2^-24 * 3 is not representable: separate rounding gives ((1 * 1 + 2^-24 * 1) -> 1) + 2^-24 * 1 -> 1, a fused or exact sum more
    e = np.float32(2.0 ** -24)
    w = rr.world([1, e, e, 0, 0, 0, 0, 0, 0], [0, 0, 0], [1, 1, 1])
    assert w[0] == np.float32(1.0)
    assert (-3 + 0) // 2 == -2
