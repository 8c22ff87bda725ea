"""The binding lifecycle and the bind-or-retry update of the subject trackers (DESIGN.md sections 29 and 30) that are plain functions
of depthhead_amd/csrc/dh_fit.h -- dh_subject_lifecycle, dh_subject_bind_or_retry, dh_subject_unbind, dh_sat_inc -- and the decision
over a row of multi-view scores, checked by tests/host/subject_bind_check.cpp, a stand-alone program with its own main: built by
plain g++ once as it is and once with -fsanitize=address,undefined, and run, the way tests/test_ident_host.py runs its program.
The kernels compile the very same functions.  Nothing of HIP is linked or run, and nothing is loaded into Python.  No GPU."""
import os
import shutil
import subprocess

import pytest

from test_ident_host import CSRC, ROOT, hip_include, sanitizer_available


def build(tmp_path, sanitize=None):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    if sanitize and not sanitizer_available(gxx, tmp_path, sanitize):
        pytest.skip(f"g++ cannot link a program with -fsanitize={sanitize}")
    exe = str(tmp_path / ("subject_bind_check" + ("_san" if sanitize else "")))
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-isystem", hip_include(),
           os.path.join(ROOT, "tests", "host", "subject_bind_check.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = [f"-fsanitize={sanitize}", "-fno-sanitize-recover=undefined"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stdout.startswith("ok ") and int(res.stdout.split()[1]) > 50000, res.stdout
    return res.stdout


def test_the_lifecycle_and_the_decision_against_the_headers_text(tmp_path):
    run(build(tmp_path))


def test_the_same_under_asan_ubsan(tmp_path):
    run(build(tmp_path, "address,undefined"))
