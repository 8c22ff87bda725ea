"""The host-only logic of the runtime (depthhead_amd/csrc/dh_host.cpp, dh_biwi.cpp: forest validation, knob parsing, tile
selection, upload chunk plans, run-length payload validation / packing, the exception guard, dh_parallel_for_) under the CPU
sanitizers: tests/host/host_check.cpp built with g++ -fsanitize=address,undefined and once more with -fsanitize=thread.
(GPU AddressSanitizer is not available on the pool; sanitizers run on the CPU build only.)"""
import os
import platform
import shutil
import subprocess

import numpy as np

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depthhead_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "host", "host_check.cpp"), os.path.join(CSRC, "dh_host.cpp"), os.path.join(CSRC, "dh_biwi.cpp")]


def _build_and_run(tmp_path, sanitize, env_extra, fixed_layout=False):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", f"-fsanitize={sanitize}",
           "-fno-sanitize-recover=undefined", "-pthread", *SOURCES, "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0 and ("cannot find -l" in res.stderr or "unrecognized" in res.stderr):
        pytest.skip(f"sanitizer runtime for {sanitize} not installed: {res.stderr[-200:]}")
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, **env_extra)
    for k in [k for k in env if k.startswith("DH_")]:
        env.pop(k)
    argv = [exe]
    if fixed_layout and shutil.which("setarch"):
        # ThreadSanitizer's runtime (gcc 11) only knows the address-space layout of up to 28 bits of mmap randomisation; on
        # kernels set to more it dies before main ("FATAL: ThreadSanitizer: unexpected memory mapping", or a bare SIGSEGV).
        # `setarch -R` turns randomisation off for this one process
        argv = [shutil.which("setarch"), platform.machine(), "-R", exe]
    run = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0 and "host_check ok" in run.stdout, (run.stdout[-2000:], run.stderr[-6000:])


def test_host_logic_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "address,undefined", {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})


def test_host_logic_under_tsan(tmp_path):
    _build_and_run(tmp_path, "thread", {"HOST_CHECK_LIGHT": "1", "TSAN_OPTIONS": "halt_on_error=1"}, fixed_layout=True)


def test_host_translation_units_have_no_hip_in_them():
    """dh_host.cpp / dh_host.h / dh_biwi.cpp stay buildable by a plain C++ compiler: no HIP header, type or call."""
    for fn in ("dh_host.cpp", "dh_host.h", "dh_biwi.cpp"):
        txt = open(os.path.join(CSRC, fn)).read()
        for word in ("hip/hip_runtime", "hipMalloc", "hipStream", "hipError_t", "__global__", "__device__", "dh_internal.h"):
            assert word not in txt, (fn, word)


_CELL_FAST_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "dh_host.h"
int main(int argc, char **argv) {          // w h k0 .. k8 -> 1 / 0
    float K[9];
    for (int i = 0; i < 9; ++i) K[i] = strtof(argv[3 + i], nullptr);
    printf("%d\n", dh_vote_cell_fast_(K, atoi(argv[1]), atoi(argv[2])) ? 1 : 0);
    return 0;
}
"""


def test_vote_cell_fast_keeps_the_benchmark_intrinsics(tmp_path):
    """dh_vote_cell_fast_ (dh_host.h) on the Python side's own matrices: the benchmark's K (synth.default_intrinsic(640, 480))
    and the principal point two frame widths beside the frame keep k_vote's approximate cell quotient; the one about 100 frame
    widths away, where the quotient is known to pick wrong cells (tests/edge_families.py), does not."""
    import edge_families as ef
    from depthhead_amd import synth
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src, exe = tmp_path / "cell_fast.cpp", str(tmp_path / "cell_fast")
    src.write_text(_CELL_FAST_DRIVER)
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-ffp-contract=off", "-pthread", f"-I{CSRC}", str(src), os.path.join(CSRC, "dh_host.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]

    def fast(K, w, h):
        args = [repr(float(v)) for v in np.asarray(K, dtype=np.float32).reshape(-1)]   # (repr of a float32 widened: exact)
        return subprocess.run([exe, str(w), str(h), *args], capture_output=True, text=True, timeout=60).stdout.strip() == "1"
    assert fast(synth.default_intrinsic(640, 480), 640, 480)
    for name, expect in (("principal_point_beside_the_frame", True), ("principal_point_far_off_the_frame", False)):
        fam = ef.FAMILIES[name]()
        n, h, w = fam.frames.shape
        assert fast(fam.K, w, h) == expect, name
