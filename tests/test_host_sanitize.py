"""The host-only logic of the runtime (depthhead_amd/csrc/dh_host.cpp, dh_biwi.cpp: forest validation, knob parsing, tile
selection, upload chunk plans, run-length payload validation / packing, the exception guard, dh_parallel_for_) under the CPU
sanitizers: tests/host/host_check.cpp built with g++ -fsanitize=address,undefined and once more with -fsanitize=thread.
(GPU AddressSanitizer is not available on the pool; sanitizers run on the CPU build only.)"""
import os

import numpy as np

import host_program as hp

CSRC = hp.CSRC
SOURCES = [hp.host("host_check.cpp"), *hp.csrc("dh_host.cpp", "dh_biwi.cpp")]


def _build_and_run(tmp_path, sanitize, env=None, fixed_layout=False):
    exe = hp.build(tmp_path, "host_check", SOURCES, sanitize, ("-pthread",))
    assert "host_check ok" in hp.run(exe, timeout=600, env=env, fixed_layout=fixed_layout).stdout


def test_host_logic_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "address,undefined")


def test_host_logic_under_tsan(tmp_path):
    _build_and_run(tmp_path, "thread", {"HOST_CHECK_LIGHT": "1"}, fixed_layout=True)


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
    src = tmp_path / "cell_fast.cpp"
    src.write_text(_CELL_FAST_DRIVER)
    exe = hp.build(tmp_path, "cell_fast", [src, *hp.csrc("dh_host.cpp")], extra=("-pthread", f"-I{CSRC}"))

    def fast(K, w, h):
        args = [repr(float(v)) for v in np.asarray(K, dtype=np.float32).reshape(-1)]   # (repr of a float32 widened: exact)
        return hp.run(exe, timeout=60, args=(w, h, *args)).stdout.strip() == "1"
    assert fast(synth.default_intrinsic(640, 480), 640, 480)
    for name, expect in (("principal_point_beside_the_frame", True), ("principal_point_far_off_the_frame", False)):
        fam = ef.FAMILIES[name]()
        n, h, w = fam.frames.shape
        assert fast(fam.K, w, h) == expect, name
