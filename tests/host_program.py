"""The one builder and the one runner of the stand-alone host programs (tests/host/*.cpp and the throw-away programs a test writes
itself).  Every program built here has its own main and is run as a process of its own: nothing is loaded
into Python.  One skip rule: no g++, or g++ cannot build and link a trivial program with the sanitizer asked for.  After that the
program under test must build -- a build error is a failure whatever its text says."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depthhead_amd", "csrc")
WARN = ("-Wall", "-Werror")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")


def host(name):
    """The path of tests/host/`name`."""
    return os.path.join(ROOT, "tests", "host", name)


def csrc(*names):
    """The paths of the library's sources `names`."""
    return [os.path.join(CSRC, n) for n in names]


def hip_include():
    """The HIP headers beside the hipcc that build() uses."""
    from depthhead_amd import build as dh_build
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(dh_build.hipcc()))), "include")
    assert os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")), inc
    return inc


def fit_header_flags():
    """What a program that includes dh_fit.h adds: the header declares the kernels' launchers, so the HIP headers are on the path
    (nothing of HIP is linked or run)."""
    return (*WARN, "-D__HIP_PLATFORM_AMD__", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-isystem", hip_include())


def sanitizer_available(gxx, tmp_path, sanitize):
    """Whether g++ can build and link a trivial program with -fsanitize=`sanitize`: asked BEFORE the program under test is built, so
    that a failure to build that program is never taken for a missing runtime."""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run([gxx, f"-fsanitize={sanitize}", str(src), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0


def build(tmp_path, name, sources, sanitize=None, extra=()):
    """The program `name` in tmp_path from `sources`, with the caller's own flags in `extra`: its path."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    if sanitize and not sanitizer_available(gxx, tmp_path, sanitize):
        pytest.skip(f"g++ cannot link a program with -fsanitize={sanitize}")
    exe = str(tmp_path / (name + ("_san" if sanitize else "")))
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off"]
    if sanitize:
        cmd += [f"-fsanitize={sanitize}", "-fno-sanitize-recover=undefined"]
    res = subprocess.run([*cmd, *extra, *map(str, sources), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def run(exe, min_ok=None, stdin=None, timeout=300, args=(), env=None, fixed_layout=False):
    """Runs `exe` with the sanitizers' options set and none of the library's DH_ knobs, requires exit status 0 and, with `min_ok`, an
    "ok <count>" on stdout with count > min_ok: the completed process (stdout and stderr as bytes where `stdin` is bytes).
    fixed_layout: ThreadSanitizer's runtime (gcc 11) only knows the address-space layout of up to 28 bits of mmap randomisation; on
    kernels set to more it dies before main ("FATAL: ThreadSanitizer: unexpected memory mapping", or a bare SIGSEGV).  `setarch -R`
    turns randomisation off for this one process."""
    full = {k: v for k, v in os.environ.items() if not k.startswith("DH_")}
    full.update(SAN_ENV, **(env or {}))
    argv = [exe, *map(str, args)]
    if fixed_layout and shutil.which("setarch"):
        argv[:0] = [shutil.which("setarch"), platform.machine(), "-R"]
    res = subprocess.run(argv, input=stdin, capture_output=True, text=not isinstance(stdin, bytes), timeout=timeout, env=full)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-6000:])
    if min_ok is not None:
        assert res.stdout.startswith("ok ") and int(res.stdout.split()[1]) > min_ok, res.stdout
    return res
