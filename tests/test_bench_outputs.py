"""bench.py --dump-outputs: what the timed path computed in its last timed step, as float .npy files, so that two builds
can be compared output for output; and --steps as the exact number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from depthhead_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poses(n, seed=5):
    from depthhead_amd._lib import POSE_DTYPE
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=POSE_DTYPE)
    p["mid_point"] = rng.integers(-500, 1500, (n, 3)).astype(np.float32)
    p["rotation"] = rng.standard_normal((n, 3))
    p["reserved"] = 7
    return p


def test_dump_outputs_writes_every_field_as_float(tmp_path):
    import bench
    p = _poses(33)
    bench.dump_outputs(str(tmp_path / "out"), p)
    assert sorted(os.listdir(tmp_path / "out")) == ["mid_point.npy", "rotation.npy"]
    mid, rot = np.load(tmp_path / "out" / "mid_point.npy"), np.load(tmp_path / "out" / "rotation.npy")
    assert mid.dtype == np.float32 and mid.shape == (33, 3) and np.array_equal(mid, p["mid_point"])
    assert rot.dtype == np.float64 and rot.shape == (33, 3) and np.array_equal(rot, p["rotation"])


def test_dump_outputs_samples_above_the_cap_the_same_way_every_time(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    p = _poses(500)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), p)
    files = {d: {f: np.load(tmp_path / d / f) for f in os.listdir(tmp_path / d)} for d in ("a", "b")}
    assert sorted(files["a"]) == ["frame_index.npy", "mid_point.npy", "rotation.npy"]
    assert sum(a.nbytes for a in files["a"].values()) <= 1000
    for f in files["a"]:
        assert files["a"][f].dtype in (np.float32, np.float64)
        assert np.array_equal(files["a"][f], files["b"][f])
    keep = files["a"]["frame_index.npy"].astype(np.int64)
    assert np.all(np.diff(keep) > 0)
    assert np.array_equal(files["a"]["mid_point.npy"], p["mid_point"][keep])
    assert np.array_equal(files["a"]["rotation.npy"], p["rotation"][keep])


@pytest.mark.parametrize("flag,value", [("--steps", "0"), ("--steps", "-3"), ("--warmup", "-1")])
def test_bench_refuses_step_counts_it_cannot_time(flag, value):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), flag, value], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert res.returncode == 2 and flag in res.stderr, res.stderr[-2000:]


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_timed_step(oracle, hip_lib, tmp_path):
    """A small bench run: the result line counts exactly --steps timed steps and the dumped outputs are the oracle's poses
    for the batch its last timed step processed."""
    nf, w, h, trees, depth, steps = 12, 320, 240, 6, 10, 7
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", str(nf), "--width", str(w), "--height", str(h),
           "--trees", str(trees), "--depth", str(depth), "--steps", str(steps), "--warmup", "2", "--no-cpu-baseline", "--no-extras",
           "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == steps and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(nf * 1e3 / out["ms_per_step"], rel=1e-2)
    assert sorted(os.listdir(out_dir)) == ["mid_point.npy", "rotation.npy"]
    mid, rot = np.load(out_dir / "mid_point.npy"), np.load(out_dir / "rotation.npy")
    assert mid.dtype == np.float32 and mid.shape == (nf, 3) and rot.dtype == np.float64 and rot.shape == (nf, 3)
    forest = synth.fit_forest(trees, depth, synth.FOREST_SEED_BASE + 2)
    K = synth.default_intrinsic(w, h)
    frames = synth.biwi_batch(nf, w, h, first=0) if out["last_step_batch"] == "a" else np.roll(synth.biwi_batch(nf, w, h, first=10000), 7, axis=0)
    ref = oracle.predict_batch(forest, synth.ModelParams(stepwidth=4), frames, K)
    assert np.array_equal(mid, ref["mid_point"]) and np.array_equal(rot, ref["rotation"])
