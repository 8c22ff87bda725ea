"""Camera rigs: heads fused across cameras into tracks with rig-wide ids (dh_rig_*, dh_rig_tracker_*) on the GPU.

Sequences of 12 steps on the composited two-head frames of test_gpu_multi_tracker.py.  The cameras of a rig see the rig's scene
(one stream frame beside another that moves 2 pixels per step); each rig has a scene of its own.  Tables of several rigs (sizes
1, 2, 3, and one of 64 cameras) with R = I and translations chosen from the restatement's own world cells, so that two views of
one head lie exactly fuse_gate apart (one person) and fuse_gate + 1 apart (two persons); and a table with rotated R.  Every
step's n_heads / heads equal predict_heads_cameras byte for byte; rig_ids, n_persons, persons, the snapshots and state() equal
tests/rig_track_ref.py fed with those heads byte for byte; host steps equal device steps equal graph replays.  Present patterns:
the cameras of a rig take turns being absent (an id moves from one camera to the other), a whole rig is absent for five steps
and resumes its ids, a rig sees blank frames for five steps (coasting, expiry, rebirth); one rig is reset; both traversal paths,
forked sub-batches and resident slices of 3 frames that cut a rig of 5 cameras in three give the same bytes.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from depthhead_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rig_track_ref as rr  # noqa: E402
from test_gpu_multi_tracker import FOREST_ARGS, composite, shifted  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 128, 112
STEPS = 12
RADIUS = 30
FUSE_GATE = 100
ABSENT_RIG = (0, range(3, 8))      # (rig, steps): every camera of the rig absent
BLANK_RIG = (2, range(3, 8))       # (rig, steps): every camera of the rig sees an empty frame
RESET = (6, 1)                     # (step, rig): reset before that step


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import _lib, prediction, tracking
    return _lib, prediction, tracking


@pytest.fixture(scope="module")
def forest():
    return synth.fit_forest(*FOREST_ARGS, n_frames=12, subset=1500)


def sequence(rig_begin, steps=STEPS, first=3, blank=BLANK_RIG, frozen=ABSENT_RIG):
    """frames [steps, n_cams, H, W]: every camera of rig g sees scene g.  The scene of rig frozen[0] stands still from the step
    before frozen[1] to the step after it: what the rig sees when it comes back is what it saw last."""
    n_rigs = len(rig_begin) - 1
    a = synth.biwi_batch(n_rigs, W, H, first=first)
    b = synth.biwi_batch(n_rigs, W, H, first=first + 500)
    out = np.zeros((steps, rig_begin[-1], H, W), dtype=np.uint16)
    for k in range(steps):
        for g in range(n_rigs):
            if blank and g == blank[0] and k in blank[1]:
                continue
            kk = k
            if frozen and g == frozen[0]:
                lo, hi = frozen[1][0] - 1, frozen[1][-1] + 1
                kk = k if k <= lo else (lo if k <= hi else k - (hi - lo))
            s = W // 3 + 2 * kk
            out[k, rig_begin[g]:rig_begin[g + 1]] = composite(a[g], shifted(b[g], -s if g % 2 else s))
    return out


def presence(rig_begin, steps=STEPS, absent=ABSENT_RIG):
    """present[k][c]: the cameras of a rig of several take turns being absent (camera k % size of the rig on odd steps); every
    camera of rig absent[0] is absent at the steps absent[1]"""
    p = np.ones((steps, rig_begin[-1]), dtype=np.uint8)
    for k in range(steps):
        for g in range(len(rig_begin) - 1):
            a, b = rig_begin[g], rig_begin[g + 1]
            if b - a == 2:
                p[k, a + k % 2] = 0            # a rig of two: exactly one camera sees each step, alternating
            elif b - a > 2 and k % 2:
                p[k, a + k % (b - a)] = 0
            if absent and g == absent[0] and k in absent[1]:
                p[k, a:b] = 0
    return p


def translations(hp, cams, frames0, rig_begin, gate=FUSE_GATE):
    """t [n, 3] for R = I.  Within a rig every camera sees the same heads at the same camera-space midpoints.  In a rig of three
    or more, camera 1 is moved along x until the restatement's own world cell of the heaviest head lies exactly `gate` from
    camera 0's (fused at the boundary), camera 2 exactly gate + 1 (not fused with camera 0's), later cameras in steps of 20 mm
    up to 140 mm.  In a rig of two, whose cameras take turns, the second stands 40 mm from the first: a person handed from one
    camera to the other stays within the match gate.  -> (t, the number of cameras placed exactly)"""
    n_heads, heads = hp.predict_heads_cameras(frames0, cams, 4, RADIUS)
    t = np.zeros((rig_begin[-1], 3), dtype=np.float32)
    eye = np.eye(3, dtype=np.float32)
    exact = 0
    for g in range(len(rig_begin) - 1):
        a, b = rig_begin[g], rig_begin[g + 1]
        for c in range(a + 1, b):
            k = c - a
            if b - a == 2:
                t[c, 0] = 40
                continue
            if k > 2:
                t[c, 0] = (k % 8) * 20
                continue
            assert n_heads[a] > 0
            want = gate if k == 1 else gate + 1
            m = heads[a, 0]["pose"]["mid_point"]
            x0 = rr.cell(rr.world(eye, t[a], m)[0])
            for tx in (want, want + 1, want - 1):
                if rr.cell(rr.world(eye, (tx, 0, 0), m)[0]) - x0 == want:
                    t[c, 0] = tx
                    exact += 1
                    break
            else:
                raise AssertionError(("no translation gives the distance", want, m))
    return t, exact


class DeviceSteps:
    """Device buffers of one rig tracker's steps (torch), and their copy back."""

    def __init__(self, torch, n, n_rigs, max_heads):
        self.torch, self.n, self.ng, self.mh = torch, n, n_rigs, max_heads
        dev = torch.device("cuda", 0)
        z = lambda count, dt: torch.zeros(count, dtype=dt, device=dev)   # noqa: E731
        self.frames = torch.zeros((n, H, W), dtype=torch.int16, device=dev)
        self.present = z(n, torch.uint8)
        self.n_heads, self.heads, self.ids = z(n, torch.int32), z(n * max_heads * 80, torch.uint8), z(n * max_heads, torch.int32)
        self.n_persons, self.persons = z(n_rigs, torch.int32), z(n_rigs * 16 * 56, torch.uint8)
        self.tracks = z(n_rigs * 16 * 72, torch.uint8)

    def load(self, frames, present):
        self.frames.copy_(self.torch.from_numpy(frames.view(np.int16)))
        self.present.copy_(self.torch.from_numpy(present))

    def ptrs(self):
        return tuple(x.data_ptr() for x in (self.frames, self.n_heads, self.heads, self.ids, self.n_persons, self.persons,
                                            self.tracks, self.present))

    def out(self, _lib):
        self.torch.cuda.synchronize()
        host = lambda x: x.cpu().numpy()   # noqa: E731
        return (host(self.n_heads).view(np.uint32), host(self.heads).view(_lib.HEAD_DTYPE).reshape(self.n, self.mh),
                host(self.ids).view(np.uint32).reshape(self.n, self.mh), host(self.n_persons).view(np.uint32),
                host(self.persons).view(_lib.RIG_PERSON_DTYPE).reshape(self.ng, 16),
                host(self.tracks).view(_lib.RIG_TRACK_DTYPE).reshape(self.ng, 16))


NAMES = ("n_heads", "heads", "rig_ids", "n_persons", "persons", "tracks")


def same(a, b, what):
    for x, y, name in zip(a, b, NAMES):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, name, x, y)


def run_host(tracking, hp, rig, frames, present, max_heads=4, fuse_gate=FUSE_GATE, gate=100, max_misses=3, reset=RESET):
    outs = []
    with tracking.RigTracker(hp, rig, W, H, max_heads, RADIUS, fuse_gate, gate, max_misses) as tr:
        for k in range(len(frames)):
            if reset and k == reset[0]:
                tr.reset(reset[1])
            outs.append(tr.step(frames[k], present[k]))
        return outs, tr.state()


def check_sequence(_lib, tracking, hp, cams, rig, frames, present, max_heads=4, fuse_gate=FUSE_GATE, gate=100, max_misses=3,
                   device=True, reset=RESET):
    """Host steps against predict_heads_cameras and the restatement, device steps against the host steps.
    -> (restatement, the persons of every step)"""
    import torch
    n, ng = frames.shape[1], rig.n_rigs
    ref = rr.Restatement(rig.R, rig.t, rig.rig_begin, max_heads, fuse_gate, gate, max_misses, _lib.RIG_TRACK_DTYPE, _lib.RIG_PERSON_DTYPE)
    outs, (st_tracks, st_next) = run_host(tracking, hp, rig, frames, present, max_heads, fuse_gate, gate, max_misses, reset)
    for k in range(len(frames)):
        want_n, want = hp.predict_heads_cameras(frames[k], cams, max_heads, RADIUS)
        if reset and k == reset[0]:
            ref.reset(reset[1])
        same(outs[k], (want_n, want) + ref.step(want_n, want, present[k]), f"host step {k}")
    assert st_tracks.tobytes() == ref.tracks.tobytes() and np.array_equal(st_next, ref.next_id)
    if device:
        s = torch.cuda.current_stream().cuda_stream
        d = DeviceSteps(torch, n, ng, max_heads)
        with tracking.RigTracker(hp, rig, W, H, max_heads, RADIUS, fuse_gate, gate, max_misses) as tr:
            for k in range(len(frames)):
                if reset and k == reset[0]:
                    tr.reset(reset[1], stream=s)
                d.load(frames[k], present[k])
                p = d.ptrs()
                tr.step_device(*p[:6], tracks_ptr=p[6], present_ptr=p[7], stream=s)
                same(d.out(_lib), outs[k], f"device step {k}")
            dt, dn = tr.state()
        assert dt.tobytes() == ref.tracks.tobytes() and np.array_equal(dn, ref.next_id)
    return ref, [o[4] for o in outs], [o[3] for o in outs]


def id_moves_between_cameras(persons, n_persons, g):
    """an id of rig g seen by one camera alone at a step and by another camera alone at the next"""
    for k in range(len(persons) - 1):
        for a in persons[k][g][: n_persons[k][g]]:
            for b in persons[k + 1][g][: n_persons[k + 1][g]]:
                if a["id"] != 0 and a["id"] == b["id"] and a["n_views"] == 1 and b["n_views"] == 1 and a["views"] != b["views"]:
                    return True
    return False


def coverage(ref, persons, n_persons, what, moving_rig=1, resumed_rig=0):
    t = ref.totals
    for key in ("multi_view", "single_view", "born", "matched", "coasting", "freed"):
        assert t[key] >= 1, (what, key, t)
    assert id_moves_between_cameras(persons, n_persons, moving_rig), what
    k0, k1 = ABSENT_RIG[1][0] - 1, ABSENT_RIG[1][-1] + 1           # the absent rig resumes its ids
    before = set(int(x) for x in persons[k0][resumed_rig]["id"][: n_persons[k0][resumed_rig]]) - {0}
    after = set(int(x) for x in persons[k1][resumed_rig]["id"][: n_persons[k1][resumed_rig]]) - {0}
    assert before and before & after, (what, before, after)
    for k in ABSENT_RIG[1]:
        assert n_persons[k][resumed_rig] == 0 and not persons[k][resumed_rig]["id"].any()


def table(tracking, hp, rig_begin, frames0, R=None):
    K0 = synth.default_intrinsic(W, H).astype(np.float32)
    cams = tracking.Cameras(np.repeat(K0[None], rig_begin[-1], axis=0))
    t, exact = translations(hp, cams, frames0, rig_begin)
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(9), (rig_begin[-1], 1))
    return cams, tracking.Rig(cams, eye if R is None else R, t, rig_begin), exact


@pytest.mark.parametrize("mode", ["plain", "general", "forked", "plain64"])
def test_steps_match_heads_and_restatement(mods, forest, monkeypatch, mode):
    _lib, prediction, tracking = mods
    if mode == "general":
        monkeypatch.setenv("DH_FORCE_GENERAL", "1")
    big = mode in ("forked", "plain64")                                    # with a rig of 64 cameras, forked and not
    rig_begin = [0, 1, 3, 6, 70] if big else [0, 1, 3, 6]
    frames = sequence(rig_begin)
    present = presence(rig_begin)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp:
        if mode == "forked":
            hp.set_forking(2)
        cams, rig, exact = table(tracking, hp, rig_begin, frames[0])
        with cams, rig:
            ref, persons, n_persons = check_sequence(_lib, tracking, hp, cams, rig, frames, present)
            if mode == "general":
                assert hp.debug_geometry()["uniform"] == 0
    assert exact >= 2, exact
    # step 0, rig 2 (cameras 3, 4, 5 all present): camera 4 at exactly fuse_gate is fused with camera 3, camera 5 at fuse_gate + 1
    # founds its own person
    p0 = persons[0][2][: n_persons[0][2]]
    assert any(p["views"] & 3 == 3 for p in p0) and any(p["views"] & 5 == 4 for p in p0), p0
    if big:
        assert max(int(p["n_views"]) for ps in persons for p in ps[3]) >= 32                  # the rig of 64: a person of many
        assert max(int(n[3]) for n in n_persons) >= 3                                         # views, several persons, and every
        assert all(int(p["n_views"]) <= 63 for p in persons[1][3])                            # odd step one camera absent
    coverage(ref, persons, n_persons, mode)


def test_rotated_extrinsics_and_other_gates(mods, forest):
    """R genuinely rotated (30 degrees about y in f32, an exact quarter turn, a scaled shear), max_heads 2, fuse gate 40, gate
    40, max_misses 0: the GPU's separately rounded transform equals the restatement's bit for bit."""
    _lib, prediction, tracking = mods
    rig_begin = [0, 3, 5]
    c, s = np.float32(np.cos(np.pi / 6)), np.float32(np.sin(np.pi / 6))
    R = np.array([[c, 0, s, 0, 1, 0, -s, 0, c], [0, 0, 1, 0, 1, 0, -1, 0, 0], [1.25, 0.5, 0, 0, 0.75, 0, 0.1, 0, 1],
                  [1, 0, 0, 0, 1, 0, 0, 0, 1], [c, -s, 0, s, c, 0, 0, 0, 1]], dtype=np.float32)
    frames = sequence(rig_begin, steps=8, first=11, blank=(1, range(3, 5)))
    present = presence(rig_begin, 8, absent=None)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp:
        cams, rig, _ = table(tracking, hp, rig_begin, frames[0], R=R)
        with cams, rig:
            ref, persons, n_persons = check_sequence(_lib, tracking, hp, cams, rig, frames, present, max_heads=2, fuse_gate=40,
                                                     gate=40, max_misses=0, reset=None)
    t = ref.totals
    assert t["born"] >= 1 and t["matched"] >= 1 and t["freed"] >= 1 and t["single_view"] >= 1, t
    w = np.concatenate([p["world"][:n] for ps, ns in zip(persons, n_persons) for p, n in zip(ps, ns)])
    assert len(w) and np.isfinite(w).all() and np.abs(w[:, 0]).max() > 100     # (the rotated cameras really move the midpoints)


def test_graph_replays_advance_as_direct_steps(mods, forest):
    import torch
    _lib, prediction, tracking = mods
    rig_begin = [0, 1, 3, 6]
    frames = sequence(rig_begin)
    present = presence(rig_begin)
    s = torch.cuda.current_stream().cuda_stream
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp:
        cams, rig, _ = table(tracking, hp, rig_begin, frames[0])
        ref = rr.Restatement(rig.R, rig.t, rig.rig_begin, 4, FUSE_GATE, 100, 3, _lib.RIG_TRACK_DTYPE, _lib.RIG_PERSON_DTYPE)
        g, d = DeviceSteps(torch, 6, 3, 4), DeviceSteps(torch, 6, 3, 4)
        persons, n_persons = [], []
        with cams, rig, tracking.RigTracker(hp, rig, W, H) as tg, tracking.RigTracker(hp, rig, W, H) as td:
            p = g.ptrs()
            tg.capture(*p[:6], tracks_ptr=p[6], present_ptr=p[7])
            for k in range(STEPS):
                g.load(frames[k], present[k])
                d.load(frames[k], present[k])
                hp.graph_launch(s)
                got = g.out(_lib)
                p = d.ptrs()
                td.step_device(*p[:6], tracks_ptr=p[6], present_ptr=p[7], stream=s)
                same(got, d.out(_lib), f"replay {k}")
                want_n, want = hp.predict_heads_cameras(frames[k], cams, 4, RADIUS)
                same(got, (want_n, want) + ref.step(want_n, want, present[k]), f"replay {k} restatement")
                persons.append(got[4])
                n_persons.append(got[3])
            a, b = tg.state(), td.state()
            assert a[0].tobytes() == b[0].tobytes() == ref.tracks.tobytes() and np.array_equal(a[1], b[1])
            hp.reserve(12, W + 16, H)                    # a reallocated workspace: the captured step is refused
            with pytest.raises(_lib.DepthheadError, match="DH_ESTATE"):
                hp.graph_launch(s)
    coverage(ref, persons, n_persons, "graph replays")


SLICE_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import test_gpu_rig_tracker as t
from depthhead_amd import synth, tracking
from depthhead_amd.prediction import HoughPrediction
d = np.load(sys.argv[1])
forest = synth.fit_forest(*t.FOREST_ARGS, n_frames=12, subset=1500)
with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(d['Ks']) as cams, \\
        tracking.Rig(cams, d['R'], d['t'], d['rig_begin']) as rig:
    outs, st = t.run_host(tracking, hp, rig, d['frames'], d['present'])
print(json.dumps([[x.tobytes().hex() for x in o] for o in outs] + [[x.tobytes().hex() for x in st]]))
"""


def test_resident_slices_smaller_than_a_rig(mods, forest, tmp_path):
    """DH_MAX_RESIDENT_FRAMES=3 over rigs of 2 and 5 cameras: the slices [0, 3), [3, 6), [6, 7) cut the second rig in three; the
    host step fuses once after the last slice and gives the bytes of the unsliced run."""
    _lib, prediction, tracking = mods
    rig_begin = [0, 2, 7]
    frames = sequence(rig_begin, steps=8, blank=(1, range(2, 6)))
    present = presence(rig_begin, 8, absent=None)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp:
        cams, rig, _ = table(tracking, hp, rig_begin, frames[0])
        with cams, rig:
            np.savez(str(tmp_path / "in.npz"), frames=frames, present=present, Ks=cams.K, R=rig.R, t=rig.t, rig_begin=rig.rig_begin)
            env = dict(os.environ, DH_MAX_RESIDENT_FRAMES="3")
            res = subprocess.run([sys.executable, "-c", SLICE_CHILD, str(tmp_path / "in.npz"), os.path.dirname(os.path.abspath(__file__))],
                                 capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
            assert res.returncode == 0, res.stderr[-3000:]
            got = json.loads(res.stdout.strip().splitlines()[-1])
            outs, st = run_host(tracking, hp, rig, frames, present)
            ref, persons, n_persons = check_sequence(_lib, tracking, hp, cams, rig, frames, present, device=False)
    want = [[x.tobytes().hex() for x in o] for o in outs] + [[x.tobytes().hex() for x in st]]
    assert got == want
    assert max(int(p["n_views"]) for ps in persons for p in ps[1]) >= 3      # persons fused across the slices' boundaries
    assert ref.totals["freed"] >= 1 and ref.totals["coasting"] >= 1, ref.totals


def test_rig_create_refusals_on_the_device(mods):
    _lib, prediction, tracking = mods
    K0 = synth.default_intrinsic(W, H).astype(np.float32)
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(9), (70, 1))
    t = np.zeros((70, 3), dtype=np.float32)
    with tracking.Cameras(np.repeat(K0[None], 70, axis=0)) as cams:
        for rb in ([0, 69], [1, 70], [0, 3, 3, 70], [0, 5, 4, 70], [0, 66, 70], [0, 70]):
            with pytest.raises(_lib.DepthheadError, match="DH_EINVAL"):
                tracking.Rig(cams, eye, t, rb)
        for bad in (np.nan, np.inf, -np.inf):
            r2, t2 = eye.copy(), t.copy()
            r2[13, 4] = bad
            with pytest.raises(_lib.DepthheadError, match="non-finite"):
                tracking.Rig(cams, r2, t, [0, 35, 70])
            t2[69, 2] = bad
            with pytest.raises(_lib.DepthheadError, match="non-finite"):
                tracking.Rig(cams, eye, t2, [0, 35, 70])
        with tracking.Rig(cams, eye * 2.5, t, [0, 64, 70]) as rig:      # not orthonormal, a rig of 64: accepted
            assert rig.n_rigs == 2
            with prediction.HoughPrediction(synth.fit_forest(*FOREST_ARGS, n_frames=12, subset=1500), synth.ModelParams(stepwidth=4)) as hp, \
                    tracking.RigTracker(hp, rig, W, H) as tr:
                for g in (-2, 2):
                    with pytest.raises(_lib.DepthheadError, match="DH_EINVAL"):
                        tr.reset(g)
                tr.reset(1)


def test_other_calls_unchanged_around_a_step(mods, forest):
    """predict_batch, a fresh HeadTracker, predict_heads and a fresh MultiHeadTracker give the same bytes before and after rig
    tracker steps in the same workspace."""
    _lib, prediction, tracking = mods
    rig_begin = [0, 2, 5]
    frames = sequence(rig_begin, steps=3, blank=None)
    K = prediction.IntrinsicMatrix(synth.default_intrinsic(W, H))

    def others(hp, cams):
        pb = hp.predict_batch(frames[0], K)
        with tracking.HeadTracker(hp, cams, W, H) as ht:
            p1 = ht.step(frames[0])
            p2 = ht.step(frames[1])
        hn, hh = hp.predict_heads(frames[2], K, 3, RADIUS)
        with tracking.MultiHeadTracker(hp, cams, W, H) as mt:
            m1 = mt.step(frames[0])
            m2 = mt.step(frames[1])
        return [x.tobytes() for x in (pb, p1, p2, hn, hh) + m1 + m2]

    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp:
        cams, rig, _ = table(tracking, hp, rig_begin, frames[0])
        with cams, rig:
            before = others(hp, cams)
            with tracking.RigTracker(hp, rig, W, H) as tr:
                for k in range(3):
                    tr.step(frames[k])
            after = others(hp, cams)
    assert before == after
