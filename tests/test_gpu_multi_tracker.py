"""Several heads per camera with identities across steps (dh_multi_tracker_*) on the GPU.

Sequences of 12 steps over several cameras: camera c sees stream frame first + c beside stream frame first + 500 + c, the
second moved by a third of the width plus 2 pixels per step (the composited two-head frames of test_gpu_heads.py), and
camera 0's frame is blank for five steps, so that its tracks coast and expire.  Each step's heads are held byte for byte to
predict_heads_cameras in the same process, and its ids, track records and state() to the restatement of
tests/multi_track_ref.py fed with those heads.  Host steps equal device steps and graph replays; forked sub-batches, resident
slices of 3 frames (a child process with DH_MAX_RESIDENT_FRAMES=3) and DH_FORCE_GENERAL=1 give the same bytes; present
patterns and the reset of one camera behave as specified; predict_batch, HeadTracker and predict_heads give the same bytes
around a multi-tracker step.  The sequences reach a birth, a match, coasting, an expiry and a refused head.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from depthhead_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multi_track_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOREST_ARGS = (6, 10, synth.FOREST_SEED_BASE + 9)
W, H = 128, 112
STEPS = 12
RADIUS = 30
BLANK = range(3, 8)            # steps at which camera 0 sees an empty frame
RESET = (6, 1)                 # (step, camera): reset before that step


@pytest.fixture(scope="module")
def mods(hip_lib):
    from depthhead_amd import _lib, prediction, tracking
    return _lib, prediction, tracking


@pytest.fixture(scope="module")
def forest():
    return synth.fit_forest(*FOREST_ARGS, n_frames=12, subset=1500)


def composite(a, b):
    both = (a > 0) & (b > 0)
    return np.where(both, np.minimum(a, b), np.maximum(a, b)).astype(np.uint16)


def shifted(img, s):
    """img moved right by s pixels (left for s < 0), zero where it leaves."""
    out = np.zeros_like(img)
    w = img.shape[1]
    if s >= 0:
        out[:, s:] = img[:, : w - s]
    else:
        out[:, : w + s] = img[:, -s:]
    return out


def sequence(n_cams, steps=STEPS, first=0, w=W, h=H, blank=BLANK):
    """frames [steps, n_cams, h, w]"""
    a = synth.biwi_batch(n_cams, w, h, first=first)
    b = synth.biwi_batch(n_cams, w, h, first=first + 500)
    out = np.empty((steps, n_cams, h, w), dtype=np.uint16)
    for k in range(steps):
        for c in range(n_cams):
            s = w // 3 + 2 * k
            out[k, c] = composite(a[c], shifted(b[c], -s if c % 2 else s))
        if k in blank:
            out[k, 0] = 0
    return out


def presence(n_cams, steps=STEPS):
    """present[k][c]: absent when (k + c) % 5 == 3, except camera 0 (whose blank steps must count as misses)"""
    p = np.ones((steps, n_cams), dtype=np.uint8)
    for k in range(steps):
        for c in range(1, n_cams):
            p[k, c] = 0 if (k + c) % 5 == 3 else 1
    return p


def cameras_k(n, w=W, h=H):
    K0 = synth.default_intrinsic(w, h).astype(np.float32)
    Ks = np.repeat(K0[None], n, axis=0)
    for i in range(1, n, 2):
        Ks[i, 0, 0] *= 1.05
        Ks[i, 1, 1] *= 1.05
        Ks[i, 0, 2] += 2
    return Ks


class DeviceSteps:
    """Device buffers of one tracker's steps (torch), and their copy back."""

    def __init__(self, torch, n, max_heads, w=W, h=H):
        self.torch, self.n, self.mh = torch, n, max_heads
        dev = torch.device("cuda", 0)
        self.frames = torch.zeros((n, h, w), dtype=torch.int16, device=dev)
        self.present = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.n_heads = torch.zeros(n, dtype=torch.int32, device=dev)
        self.heads = torch.zeros(n * max_heads * 80, dtype=torch.uint8, device=dev)
        self.ids = torch.zeros(n * max_heads, dtype=torch.int32, device=dev)
        self.tracks = torch.zeros(n * 8 * 96, dtype=torch.uint8, device=dev)

    def load(self, frames, present):
        self.frames.copy_(self.torch.from_numpy(frames.view(np.int16)))
        self.present.copy_(self.torch.from_numpy(present))

    def ptrs(self):
        return (self.frames.data_ptr(), self.n_heads.data_ptr(), self.heads.data_ptr(), self.ids.data_ptr(),
                self.tracks.data_ptr(), self.present.data_ptr())

    def out(self, _lib):
        self.torch.cuda.synchronize()
        return (self.n_heads.cpu().numpy().view(np.uint32), self.heads.cpu().numpy().view(_lib.HEAD_DTYPE).reshape(self.n, self.mh),
                self.ids.cpu().numpy().view(np.uint32).reshape(self.n, self.mh),
                self.tracks.cpu().numpy().view(_lib.TRACK_DTYPE).reshape(self.n, 8))


def same(a, b, what):
    for x, y, name in zip(a, b, ("n_heads", "heads", "ids", "tracks")):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, name, x, y)


def run_host(tracking, hp, cams, frames, present, max_heads=4, gate=100, max_misses=3, reset=RESET):
    """Host steps of a fresh tracker: the outputs of every step and the final state."""
    outs = []
    with tracking.MultiHeadTracker(hp, cams, frames.shape[3], frames.shape[2], max_heads, RADIUS, gate, max_misses) as tr:
        for k in range(len(frames)):
            if reset and k == reset[0]:
                tr.reset(reset[1])
            outs.append(tr.step(frames[k], present[k]))
        return outs, tr.state()


def check_sequence(_lib, tracking, prediction, hp, cams, frames, present, max_heads=4, gate=100, max_misses=3, device=True):
    """Host steps against predict_heads_cameras and the restatement, device steps against the host steps.  -> restatement."""
    import torch
    n = frames.shape[1]
    ref = mr.Restatement(n, max_heads, gate, max_misses, _lib.TRACK_DTYPE)
    outs, (st_tracks, st_next) = run_host(tracking, hp, cams, frames, present, max_heads, gate, max_misses)
    for k in range(len(frames)):
        want_n, want = hp.predict_heads_cameras(frames[k], cams, max_heads, RADIUS)
        n_heads, heads, ids, tracks = outs[k]
        assert n_heads.tobytes() == want_n.tobytes() and heads.tobytes() == want.tobytes(), k
        if k == RESET[0]:
            ref.reset(RESET[1])
        ref_ids, ref_tracks = ref.step(want_n, want, present[k])
        assert np.array_equal(ids, ref_ids), (k, ids, ref_ids)
        assert tracks.tobytes() == ref_tracks.tobytes(), k
    assert st_tracks.tobytes() == ref.tracks.tobytes() and np.array_equal(st_next, ref.next_id)
    if device:
        s = torch.cuda.current_stream().cuda_stream
        d = DeviceSteps(torch, n, max_heads, frames.shape[3], frames.shape[2])
        with tracking.MultiHeadTracker(hp, cams, frames.shape[3], frames.shape[2], max_heads, RADIUS, gate, max_misses) as tr:
            for k in range(len(frames)):
                if k == RESET[0]:
                    tr.reset(RESET[1], stream=s)
                d.load(frames[k], present[k])
                tr.step_device(*d.ptrs()[:5], present_ptr=d.ptrs()[5], stream=s)
                same(d.out(_lib), outs[k], f"device step {k}")
            dt, dn = tr.state()
        assert dt.tobytes() == ref.tracks.tobytes() and np.array_equal(dn, ref.next_id)
    return ref


def coverage(ref, what, expiry=True):
    t = ref.totals
    assert t["born"] >= 1 and t["matched"] >= 1 and t["coasting"] >= 1, (what, t)
    if expiry:
        assert t["freed"] >= 1, (what, t)


@pytest.mark.parametrize("mode", ["plain", "general", "forked"])
def test_steps_match_heads_and_restatement(mods, forest, monkeypatch, mode):
    _lib, prediction, tracking = mods
    if mode == "general":
        monkeypatch.setenv("DH_FORCE_GENERAL", "1")
    n = 32 if mode == "forked" else 5
    frames = sequence(n, first=3)
    present = presence(n)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(cameras_k(n)) as cams:
        if mode == "forked":
            hp.set_forking(2)
        ref = check_sequence(_lib, tracking, prediction, hp, cams, frames, present)
        if mode == "general":
            assert hp.debug_geometry()["uniform"] == 0
    coverage(ref, mode)


def test_max_heads_two_and_absent_cameras(mods, forest):
    """max_heads 2, gate 40, max_misses 0: heads arrays of stride 2; an all-absent step leaves every track as it was."""
    _lib, prediction, tracking = mods
    n = 4
    frames = sequence(n, steps=8, first=11)
    present = presence(n, 8)
    present[4] = 0
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(cameras_k(n)) as cams:
        outs, _ = run_host(tracking, hp, cams, frames, present, max_heads=2, gate=40, max_misses=0)
        assert not outs[4][2].any()
        assert outs[4][3].tobytes() == outs[3][3].tobytes()
        ref = check_sequence(_lib, tracking, prediction, hp, cams, frames, present, max_heads=2, gate=40, max_misses=0)
    coverage(ref, "max_heads 2")


def test_slot_exhaustion(mods, forest):
    """gate 0 with unrelated scenes every step and a large max_misses: every head is born, until the 8 slots are full and
    further heads are refused (id 0)."""
    _lib, prediction, tracking = mods
    n, steps = 3, 24
    frames = np.stack([sequence(n, steps=1, first=40 + 17 * k, blank=())[0] for k in range(steps)])
    present = np.ones((steps, n), dtype=np.uint8)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(cameras_k(n)) as cams:
        ref = check_sequence(_lib, tracking, prediction, hp, cams, frames, present, gate=0, max_misses=1000)
    assert ref.totals["refused"] >= 1 and ref.totals["born"] >= 8 and ref.totals["freed"] == 0, ref.totals


def test_graph_replays_advance_as_direct_steps(mods, forest):
    import torch
    _lib, prediction, tracking = mods
    n = 5
    frames = sequence(n, first=21)
    present = presence(n)
    s = torch.cuda.current_stream().cuda_stream
    ref = mr.Restatement(n, 4, 100, 3, _lib.TRACK_DTYPE)
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(cameras_k(n)) as cams:
        g, d = DeviceSteps(torch, n, 4), DeviceSteps(torch, n, 4)
        with tracking.MultiHeadTracker(hp, cams, W, H, 4, RADIUS) as tg, tracking.MultiHeadTracker(hp, cams, W, H, 4, RADIUS) as td:
            tg.capture(*g.ptrs()[:5], present_ptr=g.ptrs()[5])
            for k in range(STEPS):
                g.load(frames[k], present[k])
                d.load(frames[k], present[k])
                hp.graph_launch(s)
                got = g.out(_lib)
                td.step_device(*d.ptrs()[:5], present_ptr=d.ptrs()[5], stream=s)
                same(got, d.out(_lib), f"replay {k}")
                want_n, want = hp.predict_heads_cameras(frames[k], cams, 4, RADIUS)
                same(got[:2], (want_n, want), f"replay {k} heads")
                ids, tracks = ref.step(want_n, want, present[k])
                same(got[2:], (ids, tracks), f"replay {k} restatement")
            a, b = tg.state(), td.state()
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
            hp.reserve(2 * n, W + 16, H)                 # a reallocated workspace: the captured step is refused
            with pytest.raises(_lib.DepthheadError, match="DH_ESTATE"):
                hp.graph_launch(s)
    coverage(ref, "graph replays")


SLICE_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import test_gpu_multi_tracker as t
from depthhead_amd import synth, tracking
from depthhead_amd.prediction import HoughPrediction
d = np.load(sys.argv[1])
forest = synth.fit_forest(*t.FOREST_ARGS, n_frames=12, subset=1500)
with HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(d['Ks']) as cams:
    outs, st = t.run_host(tracking, hp, cams, d['frames'], d['present'])
print(json.dumps([[x.tobytes().hex() for x in o] for o in outs] + [[x.tobytes().hex() for x in st]]))
"""


def test_resident_slices_of_three(mods, forest, tmp_path):
    _lib, prediction, tracking = mods
    n = 7
    frames = sequence(n, steps=6, first=50, blank=range(2, 6))
    present = presence(n, 6)
    Ks = cameras_k(n)
    np.savez(str(tmp_path / "in.npz"), frames=frames, present=present, Ks=Ks)
    env = dict(os.environ, DH_MAX_RESIDENT_FRAMES="3")
    res = subprocess.run([sys.executable, "-c", SLICE_CHILD, str(tmp_path / "in.npz"), os.path.dirname(os.path.abspath(__file__))],
                         capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(Ks) as cams:
        outs, st = run_host(tracking, hp, cams, frames, present)
        ref = check_sequence(_lib, tracking, prediction, hp, cams, frames, present, device=False)
    want = [[x.tobytes().hex() for x in o] for o in outs] + [[x.tobytes().hex() for x in st]]
    assert got == want
    coverage(ref, "slices of 3")


def test_other_calls_unchanged_around_a_step(mods, forest):
    """predict_batch, a fresh HeadTracker and predict_heads give the same bytes before and after multi-tracker steps in the
    same workspace."""
    _lib, prediction, tracking = mods
    n = 5
    frames = sequence(n, steps=3, first=70, blank=())
    K = prediction.IntrinsicMatrix(synth.default_intrinsic(W, H))

    def others(hp, cams):
        pb = hp.predict_batch(frames[0], K)
        with tracking.HeadTracker(hp, cams, W, H) as ht:
            p1 = ht.step(frames[0])
            p2 = ht.step(frames[1])
        hn, hh = hp.predict_heads(frames[2], K, 3, RADIUS)
        return [x.tobytes() for x in (pb, p1, p2, hn, hh)]

    with prediction.HoughPrediction(forest, synth.ModelParams(stepwidth=4)) as hp, tracking.Cameras(cameras_k(n)) as cams:
        before = others(hp, cams)
        with tracking.MultiHeadTracker(hp, cams, W, H) as tr:
            for k in range(3):
                tr.step(frames[k])
        after = others(hp, cams)
    assert before == after
