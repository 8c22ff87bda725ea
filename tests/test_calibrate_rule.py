"""The plain functions of a calibration step (depthhead_amd/csrc/dh_fit.h) -- dh_calib_skip, the
whole-instance test of the host loop and of k_calib_accumulate, and dh_calib_pair, the test of one (instance, view) pair with
the composite pose and pivot it hands on -- checked on the host by tests/host/calib_check.cpp, a stand-alone program with its own
main: built by plain g++ once as it is and once with -fsanitize=address,undefined, and run.  dh_fit.h declares the kernels'
launchers, so the HIP headers are on the include path (beside the hipcc that build() uses); nothing of HIP is linked or run, and
nothing is loaded into Python.  No GPU."""
import os
import shutil
import subprocess

import pytest

from depthhead_amd import build as dh_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depthhead_amd", "csrc")


def hip_include():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(dh_build.hipcc()))), "include")
    assert os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")), inc
    return inc


def build(tmp_path, sanitize=None):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / ("calib_check" + ("_san" if sanitize else "")))
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-isystem", hip_include(),
           os.path.join(ROOT, "tests", "host", "calib_check.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = [f"-fsanitize={sanitize}", "-fno-sanitize-recover=undefined"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0 and sanitize and ("cannot find -l" in res.stderr or "unrecognized" in res.stderr):
        pytest.skip(f"sanitizer runtime for {sanitize} not installed: {res.stderr[-200:]}")
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stdout.startswith("ok ") and int(res.stdout.split()[1]) > 150, res.stdout
    return res.stdout


def test_the_instance_and_pair_tests_on_the_host(tmp_path):
    run(build(tmp_path))


def test_the_same_under_asan_ubsan(tmp_path):
    run(build(tmp_path, "address,undefined"))
