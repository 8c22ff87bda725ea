"""The host half of the trainer (depthhead_amd/csrc/dh_train.cpp) under the CPU sanitizers: tests/host/train_check.cpp built
with g++ -fsanitize=address,undefined and once more with -fsanitize=thread, as tests/test_host_sanitize.py does for
dh_host.cpp."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depthhead_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "host", "train_check.cpp"), os.path.join(CSRC, "dh_train.cpp"),
           os.path.join(CSRC, "dh_host.cpp"), os.path.join(CSRC, "dh_biwi.cpp")]


def _build_and_run(tmp_path, sanitize, env_extra, fixed_layout=False):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "train_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", f"-fsanitize={sanitize}",
           "-fno-sanitize-recover=undefined", "-pthread", *SOURCES, "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -l" in res.stderr or "unrecognized" in res.stderr):
        pytest.skip(f"sanitizer runtime for {sanitize} not installed: {res.stderr[-200:]}")
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, **env_extra)
    argv = [exe]
    if fixed_layout and shutil.which("setarch"):
        argv = [shutil.which("setarch"), platform.machine(), "-R", exe]   # (see test_host_sanitize.py: TSan and mmap randomisation)
    run = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0 and "train_check ok" in run.stdout, (run.stdout[-2000:], run.stderr[-6000:])


def test_train_host_logic_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "address,undefined", {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})


def test_train_host_logic_under_tsan(tmp_path):
    _build_and_run(tmp_path, "thread", {"TRAIN_CHECK_LIGHT": "1", "TSAN_OPTIONS": "halt_on_error=1"}, fixed_layout=True)


def test_train_host_unit_has_no_hip_in_it():
    for fn in ("dh_train.cpp",):
        txt = open(os.path.join(CSRC, fn)).read()
        for word in ("hip/hip_runtime", "hipMalloc", "hipStream", "hipError_t", "__global__", "dh_internal.h"):
            assert word not in txt, (fn, word)
