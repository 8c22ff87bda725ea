"""The bind of the rig fit tracker's step in its sequential form -- dh_rig_fit_bind of
depthhead_amd/csrc/dh_rig_fit.h, what lane 0 of k_rig_fit_seed runs -- against the restatement's bind (tests/rig_fit_track_ref.py,
written from the header text in Python ints).  The header is compiled by plain g++ into tests/host/rig_fit_check.cpp, a
stand-alone program with its own main, once as it is and once with -fsanitize=address,undefined; nothing is loaded into Python.
No GPU."""
import numpy as np

import host_program as hp
import rig_fit_track_ref as rf
from depthhead_amd import _lib, synth

STATE, PERSON = _lib.RIG_FIT_STATE_DTYPE, _lib.RIG_PERSON_DTYPE
UNUSED, SEEN, UNSEEN, UNBOUND = 0, 1, 2, 3
MAX_HEADS = 2


def build(tmp_path, sanitize=None):
    return hp.build(tmp_path, "rig_fit_check", [hp.host("rig_fit_check.cpp")], sanitize, (*hp.WARN, "-I" + hp.CSRC))


def run_cases(exe, cases):
    buf = bytearray()
    for st, persons, n_persons, n_heads in cases:
        buf += np.array([n_persons, len(n_heads), MAX_HEADS], np.uint32).tobytes() + st.tobytes() + persons.tobytes() + n_heads.tobytes()
    run = hp.run(exe, stdin=bytes(buf), timeout=300)
    out, size = [], 16 * STATE.itemsize + 128
    assert len(run.stdout) == size * len(cases)
    for i in range(len(cases)):
        b = run.stdout[i * size:(i + 1) * size]
        out.append((np.frombuffer(b[:16 * STATE.itemsize], STATE), np.frombuffer(b[-128:-64], np.uint32), np.frombuffer(b[-64:], np.uint32)))
    return out


def expected(st, persons, n_persons, n_heads):
    slots, ids, founded, freed = rf.bind(st["id"].tolist(), st["tracked"].tolist(), persons, n_persons, n_heads, MAX_HEADS)
    want = st.copy()
    for s in range(16):
        if s in founded or s in freed:
            want[s] = 0
        want[s]["id"] = ids[s]
    role = [{"seen": SEEN, "unseen": UNSEEN, "unbound": UNBOUND}[x[0]] if x else UNUSED for x in slots]
    who = [x[1] if x and x[1] is not None else rf.NO_PERSON for x in slots]
    return want, role, who


def random_case(rng, n_cams=5):
    """Entries with few distinct ids, some free, some tracked; persons whose ids repeat, are 0, are unknown, or name no head."""
    def draw(k):
        return (rng.uniform(k) * 65536.0).astype(np.int64)
    st = np.zeros(16, STATE)
    ids = rng.permutation(20)[:16] + 1
    live = draw(16) % 4 != 0 if draw(1)[0] % 8 else np.ones(16, bool)
    st["id"] = np.where(live, ids, 0)
    st["tracked"] = np.where(live, draw(16) % 2, 0)
    st["age"], st["lost"], st["views_used"] = draw(16) % 9, draw(16) % 3, draw(16) % 8
    st["t"] = draw(48).reshape(16, 3) % 100
    st[~live] = 0
    persons = np.zeros(16, PERSON)
    persons["id"] = draw(16) % 24
    persons["best_cam"] = draw(16) % (n_cams + 1)              # n_cams: no camera of the table
    persons["best_head"] = draw(16) % (MAX_HEADS + 1)
    persons["views"] = draw(16) % 8
    n_heads = (draw(n_cams) % (MAX_HEADS + 2)).astype(np.uint32)
    return st, persons, int(draw(1)[0] % 19), n_heads           # n_persons up to 18: the walk stops at 16


def compare(exe, cases):
    for i, ((got_st, got_role, got_who), case) in enumerate(zip(run_cases(exe, cases), cases)):
        want_st, role, who = expected(*case)
        assert got_role.tolist() == role and got_who.tolist() == who, (i, got_role, role, got_who, who)
        assert got_st.tobytes() == want_st.tobytes(), i


def hand_cases():
    free = np.zeros(16, STATE)
    full = np.zeros(16, STATE)
    full["id"], full["tracked"] = np.arange(1, 17), 1
    untracked = full.copy()
    untracked["tracked"][[3, 9]] = 0
    nh = np.full(5, MAX_HEADS, np.uint32)

    def persons(ids, cam=0, head=0):
        p = np.zeros(16, PERSON)
        p["id"][:len(ids)] = ids
        p["best_cam"], p["best_head"] = cam, head
        return p
    return [(free, persons([]), 0, nh), (free, persons(list(range(1, 17))), 16, nh), (free, persons([5, 5, 0, 5]), 4, nh),
            (full, persons([17, 3, 18]), 3, nh), (untracked, persons([17, 18, 19, 5]), 4, nh), (untracked, persons([0] * 16), 16, nh),
            (full, persons([3, 3]), 200, nh), (free, persons([1, 2], cam=5), 2, nh), (free, persons([1, 2], head=MAX_HEADS), 2, nh),
            (free, persons([1, 2], head=1), 2, np.array([1, 2, 2, 2, 2], np.uint32)), (untracked, persons([]), 0, nh)]


def test_hand_cases_match_the_restatement(tmp_path):
    exe = build(tmp_path)
    cases = hand_cases()
    compare(exe, cases)
    out = run_cases(exe, cases)
    assert out[1][1].tolist() == [SEEN] * 16 and out[1][0]["id"].tolist() == list(range(1, 17))
    assert out[2][1][:4].tolist() == [SEEN, UNBOUND, UNBOUND, UNBOUND] and out[2][2][:4].tolist() == [0, 1, 2, 3]
    assert out[3][1].tolist() == [UNSEEN, UNSEEN, SEEN] + [UNSEEN] * 13         # ids 17 and 18: no entry and no record slot
    # ids 17, 18, 19 find no free entry in the walk; the two untracked unseen entries are freed after it and report 17 and 18
    assert out[4][1][[3, 9]].tolist() == [UNBOUND, UNBOUND] and out[4][2][[3, 9]].tolist() == [0, 1] and out[4][0]["id"][[3, 9]].tolist() == [0, 0]
    assert out[7][1].tolist() == [UNUSED] * 16 and out[8][1].tolist() == [UNUSED] * 16 and out[9][1][:2].tolist() == [UNUSED, UNUSED]


def test_random_cases_match_the_restatement(tmp_path):
    rng = synth.SplitMix(2200)

    class R:
        uniform = staticmethod(rng.uniform)

        @staticmethod
        def permutation(n):
            return np.argsort(rng.uniform(n), kind="stable")
    compare(build(tmp_path), [random_case(R) for _ in range(300)])


def test_bind_under_asan_ubsan(tmp_path):
    rng = synth.SplitMix(2201)

    class R:
        uniform = staticmethod(rng.uniform)

        @staticmethod
        def permutation(n):
            return np.argsort(rng.uniform(n), kind="stable")
    compare(build(tmp_path, "address,undefined"), hand_cases() + [random_case(R) for _ in range(100)])
