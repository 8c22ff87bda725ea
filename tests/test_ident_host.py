"""The decision of an identification that is plain functions of depthhead_amd/csrc/dh_fit.h -- the order, the
status, the mean square and the picks the decide wave keeps and merges -- checked by tests/host/ident_check.cpp, a stand-alone
program with its own main: built by plain g++ once as it is and once with -fsanitize=address,undefined, and run, the way
tests/test_surface_host.py runs its program.  The kernel compiles the very same functions.  Nothing of HIP is linked or run, and
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


def sanitizer_available(gxx, tmp_path, sanitize):
    """Whether g++ can build and link a trivial program with -fsanitize=`sanitize`: asked BEFORE the program under test is built."""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run([gxx, f"-fsanitize={sanitize}", str(src), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0


def build(tmp_path, sanitize=None):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    if sanitize and not sanitizer_available(gxx, tmp_path, sanitize):
        pytest.skip(f"g++ cannot link a program with -fsanitize={sanitize}")
    exe = str(tmp_path / ("ident_check" + ("_san" if sanitize else "")))
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-isystem", hip_include(),
           os.path.join(ROOT, "tests", "host", "ident_check.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = [f"-fsanitize={sanitize}", "-fno-sanitize-recover=undefined"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    assert res.stdout.startswith("ok ") and int(res.stdout.split()[1]) > 10000, res.stdout
    return res.stdout


def test_the_order_the_status_and_the_picks_against_a_sort(tmp_path):
    run(build(tmp_path))


def test_the_same_under_asan_ubsan(tmp_path):
    run(build(tmp_path, "address,undefined"))
