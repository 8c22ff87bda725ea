"""The host half of the trainer (depthhead_amd/csrc/dh_train.cpp) under the CPU sanitizers: tests/host/train_check.cpp built
with g++ -fsanitize=address,undefined and once more with -fsanitize=thread, as tests/test_host_sanitize.py does for
dh_host.cpp (both through tests/host_program.py)."""
import os

import host_program as hp

CSRC = hp.CSRC
SOURCES = [hp.host("train_check.cpp"), *hp.csrc("dh_train.cpp", "dh_host.cpp", "dh_biwi.cpp")]


def _build_and_run(tmp_path, sanitize, env=None, fixed_layout=False):
    exe = hp.build(tmp_path, "train_check", SOURCES, sanitize, ("-pthread",))
    assert "train_check ok" in hp.run(exe, timeout=600, env=env, fixed_layout=fixed_layout).stdout


def test_train_host_logic_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, "address,undefined")


def test_train_host_logic_under_tsan(tmp_path):
    _build_and_run(tmp_path, "thread", {"TRAIN_CHECK_LIGHT": "1"}, fixed_layout=True)   # (see host_program.run: TSan and mmap randomisation)


def test_train_host_unit_has_no_hip_in_it():
    for fn in ("dh_train.cpp",):
        txt = open(os.path.join(CSRC, fn)).read()
        for word in ("hip/hip_runtime", "hipMalloc", "hipStream", "hipError_t", "__global__", "dh_internal.h"):
            assert word not in txt, (fn, word)
