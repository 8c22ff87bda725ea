"""The multi-head tracker's step (depthhead_amd/csrc/dh_track_heads.h, the header k_track_heads is built from) against the
restatement of tests/multi_track_ref.py, step by step over hand-built and random sequences: the gate boundary, both tie
orders, crossing heads, coasting and expiry (max_misses 3 and 0), slot exhaustion and reuse, next_id wrapping, NaN / inf /
saturating midpoints, empty frames, absent cameras and saturating counters.  The header is compiled by plain g++
(tests/host/multi_track_check.cpp), and again under ASan / UBSan."""
import os
import sys

import numpy as np
import pytest

from depthhead_amd._lib import HEAD_DTYPE, TRACK_DTYPE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_program as hp  # noqa: E402
import multi_track_ref as mr  # noqa: E402

U32 = 0xFFFFFFFF
INF, NAN = float("inf"), float("nan")


def head(mid, tag=0):
    """A HEAD_DTYPE record at midpoint `mid`; every other field carries `tag`, so that a copy of the whole record shows."""
    h = np.zeros((), dtype=HEAD_DTYPE)
    h["pose"]["mid_point"] = np.asarray(mid, dtype=np.float32)
    h["pose"]["rotation"] = (0.5 * tag, -0.25 * tag, tag + 0.125)
    s = h["support"]
    s["x"], s["y"], s["width"], s["height"] = tag, tag + 1, tag + 2, tag + 3
    s["windows"], s["hits"], s["mass"], s["total_mass"] = tag + 4, tag + 5, (tag << 33) + 7, (tag << 34) + 9
    return h


def frame(mids, max_heads, tag0=0):
    """(HEAD_DTYPE [max_heads], n): the heads at `mids`, the slots after them zero."""
    hs = np.zeros(max_heads, dtype=HEAD_DTYPE)
    for j, m in enumerate(mids):
        hs[j] = head(m, tag0 + j + 1)
    return hs, len(mids)


class Seq:
    def __init__(self, name, max_heads=4, gate=100, max_misses=3, tracks=None, next_id=1):
        self.name, self.max_heads, self.gate, self.max_misses = name, max_heads, gate, max_misses
        self.tracks = np.zeros(mr.MAX_TRACKS, dtype=TRACK_DTYPE) if tracks is None else tracks
        self.next_id = next_id
        self.steps = []

    def add(self, mids, present=True, n=None):
        hs, k = frame(mids, self.max_heads, tag0=10 * len(self.steps))
        self.steps.append((hs, k if n is None else n, present))
        return self


def hand_sequences():
    z = 1000.5
    seqs = []
    # the gate: d == gate is matched, gate + 1 is not (also at gate 0)
    for g in (100, 0, 7):
        seqs.append(Seq(f"gate {g}", gate=g).add([(0.9, 0, z)]).add([(g + 0.9, 0, z)]).add([(2 * g + 1.9, -0.5, z)]))
        seqs.append(Seq(f"gate {g} z", gate=g).add([(0, 0, z)]).add([(0, -0.0, z - g - 0.5)]).add([(0, 0, z - 2 * g - 2)]))
    # ties: two heads at the same distance of one track (lower j first); one head equidistant from two tracks (lower t first)
    seqs.append(Seq("tie heads").add([(0, 0, z)]).add([(30, 0, z), (-30, 0, z)]).add([(-30, 0, z), (30, 0, z)]))
    seqs.append(Seq("tie tracks").add([(-40, 0, z), (40, 0, z)]).add([(0, 0, z)]).add([(0, 0, z), (80, 0, z)]))
    # two heads crossing: they pass each other in x (150 mm apart in y) while their order in the frame swaps; and two whose
    # paths meet, where the rule's tie order decides
    for name, dy in (("crossing", 150), ("meeting", 5)):
        s = Seq(name)
        for k in range(8):
            a, b = (-60 + 15 * k, 0, z), (60 - 15 * k, dy, z)
            s.add([a, b] if k % 3 else [b, a])
        seqs.append(s)
    # coasting, then expiry: kept at misses == max_misses, freed at max_misses + 1
    for mm in (3, 0, 1):
        s = Seq(f"expiry {mm}", max_misses=mm).add([(0, 0, z), (300, 0, z)])
        for _ in range(mm + 1):
            s.add([(300, 0, z)])
        s.add([(0, 0, z), (300, 0, z)])
        seqs.append(s)
    # slot exhaustion: 8 live tracks coasting, more heads refused (id 0); the lowest freed slot is reused
    s = Seq("exhaustion", gate=0, max_misses=2)
    s.add([(0, 0, z), (1000, 0, z), (2000, 0, z), (3000, 0, z)])
    s.add([(0, 1000, z), (1000, 1000, z), (2000, 1000, z), (3000, 1000, z)])
    s.add([(0, 2000, z), (1000, 2000, z), (2000, 2000, z), (3000, 2000, z)])
    s.add([(1000, 0, z), (0, 1000, z)])
    s.add([(1000, 0, z), (0, 1000, z), (5, 5, 5)])
    s.add([(1000, 0, z), (0, 1000, z), (5, 5, 5), (6, 6, 6)])
    seqs.append(s)
    # next_id wraps from UINT32_MAX to 1
    seqs.append(Seq("wrap", gate=0, next_id=U32 - 1).add([(0, 0, z), (500, 0, z), (900, 0, z)]).add([(0, 0, z), (0, 500, z)]))
    # NaN, +-inf and saturating midpoints (their cells: 0, INT32_MAX, INT32_MIN)
    s = Seq("non-finite", gate=5)
    s.add([(NAN, 0, z), (INF, 1e12, z), (-INF, -1e12, -3e9)])
    s.add([(0.5, NAN, z), (3e9, 2.2e9, z), (-2.2e9, -INF, -INF)])
    s.add([(NAN, NAN, NAN), (INF, INF, INF), (2147483520.0, -2147483648.0, 0)])
    seqs.append(s)
    # n_heads = 0, absent steps (state kept, ids zero), n_heads beyond max_heads (clamped)
    s = Seq("empty and absent", max_heads=2).add([(0, 0, z), (200, 0, z)]).add([]).add([(0, 0, z)], present=False)
    s.add([(900, 0, z)], present=False).add([(10, 0, z), (190, 0, z)]).add([(10, 0, z), (190, 0, z)], n=7)
    seqs.append(s)
    # saturating counters
    tr = np.zeros(mr.MAX_TRACKS, dtype=TRACK_DTYPE)
    tr[0]["id"], tr[0]["age"], tr[0]["hits"], tr[0]["misses"] = 5, U32 - 1, U32 - 1, 0
    tr[0]["head"] = head((0, 0, z), 3)
    tr[3]["id"], tr[3]["age"], tr[3]["hits"], tr[3]["misses"] = 9, U32, 17, U32 - 1
    tr[3]["head"] = head((5000, 0, z), 4)
    s = Seq("saturation", max_misses=U32, tracks=tr, next_id=10).add([(0, 0, z)]).add([(0, 0, z)]).add([(0, 0, z)])
    seqs.append(s)
    return seqs


def random_sequences(count=60, seed=11):
    rs = np.random.RandomState(seed)
    seqs = []
    for i in range(count):
        s = Seq(f"random {i}", max_heads=int(rs.randint(1, 5)), gate=int(rs.choice([0, 3, 40, 100, 2**31 - 1])),
                max_misses=int(rs.choice([0, 1, 3, 5, U32])), next_id=int(rs.choice([1, 7, U32 - 2])))
        pos = rs.uniform(-400, 400, (6, 3)) + np.array([0, 0, 1000])
        for _ in range(int(rs.randint(4, 14))):
            pos += rs.normal(0, rs.choice([5, 40, 150]), pos.shape)
            k = int(rs.randint(0, s.max_heads + 1))
            mids = [tuple(pos[q]) for q in rs.permutation(6)[:k]]
            s.add(mids, present=bool(rs.rand() > 0.15))
        seqs.append(s)
    return seqs


def _build(tmp_path, sanitize):
    return hp.build(tmp_path, "multi_track_check", [hp.host("multi_track_check.cpp")], sanitize, (*hp.WARN, "-I" + hp.CSRC))


def run_checker(exe, cases):
    """cases: (max_heads, heads, n, gate, max_misses, next_id, present, tracks) -> [(tracks, next_id, ids)]"""
    buf = bytearray()
    for mh, hs, n, gate, mm, nid, pres, tr in cases:
        buf += np.array([mh, n, gate, mm, nid, int(pres)], dtype=np.uint32).tobytes()
        buf += np.ascontiguousarray(tr).tobytes() + np.ascontiguousarray(hs).tobytes()
    run = hp.run(exe, stdin=bytes(buf), timeout=120)
    out, pos, res = run.stdout, 0, []
    for mh, *_ in cases:
        tr = np.frombuffer(out, dtype=TRACK_DTYPE, count=mr.MAX_TRACKS, offset=pos).copy()
        pos += tr.nbytes
        nid = int(np.frombuffer(out, dtype=np.uint32, count=1, offset=pos)[0])
        pos += 4
        ids = np.frombuffer(out, dtype=np.uint32, count=mh, offset=pos).copy()
        pos += 4 * mh
        res.append((tr, nid, ids))
    assert pos == len(out)
    return res


def drive(exe, seqs):
    """Every sequence step by step through the header and the restatement; both must agree on tracks, next_id and ids.
    -> per sequence the list of (ids, info, tracks) of its steps, and the totals of the restatement's info."""
    state = [(s.tracks.copy(), s.next_id) for s in seqs]
    hist = [[] for _ in seqs]
    totals = dict(matched=0, born=0, coasting=0, freed=0, refused=0)
    for k in range(max(len(s.steps) for s in seqs)):
        live = [i for i, s in enumerate(seqs) if k < len(s.steps)]
        cases = []
        for i in live:
            s = seqs[i]
            hs, n, pres = s.steps[k]
            cases.append((s.max_heads, hs, n, s.gate, s.max_misses, state[i][1], pres, state[i][0]))
        got = run_checker(exe, cases)
        for i, (tr, nid, ids) in zip(live, got):
            s = seqs[i]
            hs, n, pres = s.steps[k]
            want_tr, want_nid, want_ids, info = mr.step(state[i][0], state[i][1], hs, n, s.gate, s.max_misses, pres)
            assert tr.tobytes() == want_tr.tobytes(), (s.name, k, tr, want_tr)
            assert nid == want_nid, (s.name, k, nid, want_nid)
            assert np.array_equal(ids, want_ids), (s.name, k, ids, want_ids)
            state[i] = (tr, nid)
            hist[i].append((ids, info, tr))
            for key, v in info.items():
                totals[key] += v
    return hist, totals


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("mtc"), None)


def by_name(seqs, hist):
    return {s.name: h for s, h in zip(seqs, hist)}


def test_hand_cases_match_restatement(checker):
    seqs = hand_sequences()
    hist, totals = drive(checker, seqs)
    h = by_name(seqs, hist)
    for g in (100, 0, 7):
        ids = [x[0][0] for x in h[f"gate {g}"]]
        assert ids == [1, 1, 2], (g, ids)            # d == gate matched, gate + 1 born anew
        ids = [x[0][0] for x in h[f"gate {g} z"]]
        assert ids == [1, 1, 2], (g, ids)
    assert list(h["tie heads"][1][0][:2]) == [1, 2]    # equal d: head 0 takes the track
    assert list(h["tie heads"][2][0][:2]) == [2, 1]
    assert list(h["tie tracks"][1][0][:1]) == [1]      # equal d: slot 0 takes the head
    cr = [(int(x[0][0]), int(x[0][1])) for x in h["crossing"]]
    assert cr == [(2, 1) if k % 3 else (1, 2) for k in range(8)], cr   # ids follow the heads, not their order
    assert [int(x[0][0]) for x in h["meeting"]][4] == 1    # where the paths meet, equal d: head 0 takes slot 0 (id 1)
    for mm in (3, 0, 1):
        e = h[f"expiry {mm}"]
        for k in range(1, mm + 1):                   # coasting: kept while misses <= max_misses
            assert e[k][2][0]["id"] == 1 and e[k][2][0]["misses"] == k and e[k][2][0]["age"] == k + 1, (mm, k)
        assert e[mm + 1][2][0]["id"] == 0 and e[mm + 1][1]["freed"] == 1, mm    # freed at max_misses + 1
        assert list(e[-1][0][:2]) == [3, 2] and e[-1][2][0]["id"] == 3       # the lost head is born again in slot 0
    ex = h["exhaustion"]
    assert not ex[2][0].any() and ex[2][1]["refused"] == 4                  # a 9th track is refused: ids 0
    assert list(ex[5][0]) == [2, 5, 9, 10]
    assert list(ex[5][2]["id"]) == [9, 2, 10, 0, 5, 0, 0, 0]                # the lowest freed slots are reused
    wrap = h["wrap"]
    assert list(wrap[0][0][:3]) == [U32 - 1, U32, 1]
    assert wrap[1][0][1] == 2
    emp = h["empty and absent"]
    assert not emp[1][0].any() and not emp[2][0].any() and not emp[3][0].any()
    assert emp[2][2].tobytes() == emp[1][2].tobytes() == emp[3][2].tobytes()
    sat = h["saturation"][-1][2]
    assert sat[0]["age"] == U32 and sat[0]["hits"] == U32 and sat[3]["misses"] == U32 and sat[3]["id"] == 9
    for key in totals:
        assert totals[key] >= 1, totals


def test_random_sequences_match_restatement(checker):
    seqs = random_sequences()
    _, totals = drive(checker, seqs)
    for key in totals:
        assert totals[key] >= 5, totals


def test_rule_under_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "address,undefined")
    drive(exe, hand_sequences() + random_sequences(20, seed=5))


def test_restatement_at_its_edges():
    """The restatement itself: cells of non-finite and huge midpoints, and the exhaustion case refuses heads."""
    assert [mr.cell(v) for v in (NAN, INF, -INF, 3e9, -3e9, -0.9, 0.9, -2147483648.0)] == \
           [0, 2**31 - 1, -2**31, 2**31 - 1, -2**31, 0, 0, -2**31]
    tr = np.zeros(mr.MAX_TRACKS, dtype=TRACK_DTYPE)
    nid = 1
    refused = 0
    for k in range(3):
        hs, n = frame([(5000 * k + 1000 * j, 0, 1000) for j in range(4)], 4)
        tr, nid, ids, info = mr.step(tr, nid, hs, n, 0, 10)
        refused += info["refused"]
    assert refused == 4 and list(ids) == [0, 0, 0, 0] and nid == 9
