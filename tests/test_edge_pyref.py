"""The adversarial families of tests/edge_families.py through both CPU restatements: oracle/pyref.py (written from the Rust
text) against the C oracle (oracle/dh_oracle.c) in both rectangle modes, on every intermediate -- leaf indices, patch
flags, both guess grids, the guesses, both sparse accumulators, both mean-shift traces, the pose -- and, for the sibling
consumers, predict_mask and the u16 vote image.  Every family first asserts that it reaches its edge.

Then the oracle itself under AddressSanitizer + UndefinedBehaviorSanitizer (a CPU build, in a child process): every family
again, results equal to the normal build's."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import edge_families as ef
from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("leaf_idx", "patch_flags", "pos_grid", "rot_grid", "guess_mid", "guess_rot", "mid_cells", "rot_cells", "ms_trace_mid",
        "ms_trace_rot", "mid_point", "rotation")
MODES = {"faithful": 0, "sat": 1}

_cache = {}


def family_results(name):
    """(family, pyref results) of a 3-D family, computed once per session; the family's reach() is checked here."""
    if name not in _cache:
        fam = ef.FAMILIES[name]()
        with np.errstate(all="ignore"):
            res = [pyref.predict(fam.forest, fam.model, f, fam.K, *fam.guesses(i)) for i, f in enumerate(fam.frames)]
        fam.reach(res)
        _cache[name] = (fam, res)
    return _cache[name]


def decoy_results(name):
    """(decoy cameras, pyref results of frame i seen through decoy camera i) of a 3-D family (ef.decoy_cameras), once per session."""
    key = ("decoy", name)
    if key not in _cache:
        fam = family_results(name)[0]
        Ds = ef.decoy_cameras(fam)
        with np.errstate(all="ignore"):
            res = [pyref.predict(fam.forest, fam.model, f, Ds[i], *fam.guesses(i)) for i, f in enumerate(fam.frames)]
        _cache[key] = (Ds, res)
    return _cache[key]


def aux_family_results(name):
    key = ("aux", name)
    if key not in _cache:
        fam = ef.AUX_FAMILIES[name]()
        with np.errstate(all="ignore"):
            res = ef.aux_results(fam)
        fam.reach(res)
        _cache[key] = (fam, res)
    return _cache[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(ef.FAMILIES))
def test_pyref_against_the_oracle(oracle, name, mode):
    fam, res = family_results(name)
    for i, f in enumerate(fam.frames):
        mg, rg = fam.guesses(i)
        r = oracle.predict(fam.forest, fam.model, f, fam.K, mg, rg, rect_mode=MODES[mode])
        for k in KEYS:
            assert np.array_equal(res[i][k], getattr(r, k)), (name, i, k, res[i][k], getattr(r, k))


@pytest.mark.parametrize("name", list(ef.FAMILIES))
def test_pyref_against_the_oracle_with_decoy_cameras(oracle, name):
    """The decoy cameras that tests/test_gpu_camera_edges.py interleaves with every family's own K: pyref and the oracle agree
    on every intermediate there too."""
    fam = family_results(name)[0]
    Ds, res = decoy_results(name)
    assert ef.is_pinhole(Ds[0]) == ef.is_pinhole(fam.K) and not (Ds == fam.K).all(axis=(1, 2)).any()
    for i, f in enumerate(fam.frames):
        mg, rg = fam.guesses(i)
        r = oracle.predict(fam.forest, fam.model, f, Ds[i], mg, rg)
        for k in KEYS:
            assert np.array_equal(res[i][k], getattr(r, k)), (name, i, k, res[i][k], getattr(r, k))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(ef.AUX_FAMILIES))
def test_pyref_aux_against_the_oracle(oracle, name, mode):
    fam, res = aux_family_results(name)
    for i, f in enumerate(fam.frames):
        assert np.array_equal(res[i]["mask"], oracle.predict_mask(fam.forest, fam.model, f, rect_mode=MODES[mode])), (name, i)
        assert np.array_equal(res[i]["votes"], oracle.hough_image(fam.forest, fam.model, f, fam.K, rect_mode=MODES[mode])), (name, i)
    if mode == "sat":
        blurred = [oracle.build_hough_image(fam.forest, fam.model, f, fam.K) for f in fam.frames]
        ef.expectations(fam, blurred, fam.frames)


def test_vote_image_sums_past_65535_wrap(oracle):
    """prediction.rs:832 adds into a u16 pixel with `+=`: pixels whose true sum passed 65 535 hold the residue mod 2^16."""
    fam, res = aux_family_results("aux_vote_limits")
    over = 0
    for r in res:
        for (y, x), s in np.ndenumerate(r["sums"]):
            if s > 65535:
                over += 1
                assert r["votes"][y, x] == s % 65536
    assert over > 0


# ------------------------------------------------------------------ the oracle under ASan + UBSan
_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
from oracle import pyoracle
if sys.argv[2] != "-":
    pyoracle.use_library(sys.argv[2])
import edge_families as ef
out = {}
for name, make in ef.FAMILIES.items():
    fam = make()
    for mode in (0, 1):
        for i, f in enumerate(fam.frames):
            mg, rg = fam.guesses(i)
            r = pyoracle.predict(fam.forest, fam.model, f, fam.K, mg, rg, rect_mode=mode)
            for k in ("leaf_idx", "patch_flags", "pos_grid", "rot_grid", "guess_mid", "guess_rot", "mid_cells", "rot_cells",
                      "ms_trace_mid", "ms_trace_rot", "mid_point", "rotation"):
                out[f"{name}/{mode}/{i}/{k}"] = getattr(r, k)
    out[f"{name}/batch"] = pyoracle.predict_batch(fam.forest, fam.model, fam.frames, fam.K, fam.midp, fam.rot, threads=2)
for name, make in ef.AUX_FAMILIES.items():
    fam = make()
    for i, f in enumerate(fam.frames):
        for mode in (0, 1):
            out[f"{name}/{mode}/{i}/mask"] = pyoracle.predict_mask(fam.forest, fam.model, f, rect_mode=mode)
            out[f"{name}/{mode}/{i}/votes"] = pyoracle.hough_image(fam.forest, fam.model, f, fam.K, rect_mode=mode)
        out[f"{name}/{i}/blurred"] = pyoracle.build_hough_image(fam.forest, fam.model, f, fam.K)
        out[f"{name}/{i}/pose"] = np.concatenate(pyoracle.predict_from2dhough(fam.forest, fam.model, f, fam.K))
np.savez(sys.argv[3], **out)
print("families ok", len(out))
"""


def _run_child(tmp_path, lib, out, env):
    script = tmp_path / "families.py"
    script.write_text(_CHILD)
    run = subprocess.run([sys.executable, str(script), ROOT, lib, str(out)], capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0 and "families ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-6000:])
    return run


def test_oracle_under_asan_ubsan(tmp_path, oracle):
    """dh_oracle.c built with the flags of oracle/Makefile's `asan` rule (into tmp_path), loaded into a child Python with
    gcc's libasan preloaded, halting on the first report; every family's results equal those of the normal build."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    libasan = subprocess.run([gcc, "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("gcc's libasan is not installed")
    so = str(tmp_path / "libdh_oracle_asan.so")
    cmd = [gcc, "-O1", "-g", "-std=c11", "-ffp-contract=off", "-fPIC", "-fopenmp", "-fsanitize=address,undefined", "-shared",
           "-o", so, os.path.join(ROOT, "oracle", "dh_oracle.c"), "-lm"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -l" in res.stderr or "unrecognized" in res.stderr):
        pytest.skip(f"sanitizer runtime not installed: {res.stderr[-200:]}")
    assert res.returncode == 0, res.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DH_")}
    _run_child(tmp_path, "-", tmp_path / "plain.npz", env)
    env.update(LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    san = _run_child(tmp_path, so, tmp_path / "san.npz", env)
    assert "runtime error" not in san.stderr and "AddressSanitizer" not in san.stderr, san.stderr[-6000:]
    a, b = np.load(tmp_path / "plain.npz"), np.load(tmp_path / "san.npz")
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        x, y = a[k], b[k]
        for f in (x.dtype.names or (None,)):             # field by field: the padding of a pose record is not a result
            assert (x if f is None else x[f]).tobytes() == (y if f is None else y[f]).tobytes(), (k, f)
