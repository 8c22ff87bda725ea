"""The plain functions of a calibration step (depthhead_amd/csrc/dh_fit.h) -- dh_calib_skip, the
whole-instance test of the host loop and of k_calib_accumulate, and dh_calib_pair, the test of one (instance, view) pair with
the composite pose and pivot it hands on -- checked on the host by tests/host/calib_check.cpp, a stand-alone program with its own
main: built by plain g++ once as it is and once with -fsanitize=address,undefined, and run.  dh_fit.h declares the kernels'
launchers, so the HIP headers are on the include path (beside the hipcc that build() uses); nothing of HIP is linked or run, and
nothing is loaded into Python.  No GPU."""
import host_program as hp


def check(tmp_path, sanitize=None):
    exe = hp.build(tmp_path, "calib_check", [hp.host("calib_check.cpp")], sanitize, hp.fit_header_flags())
    hp.run(exe, min_ok=150, timeout=300)


def test_the_instance_and_pair_tests_on_the_host(tmp_path):
    check(tmp_path)


def test_the_same_under_asan_ubsan(tmp_path):
    check(tmp_path, "address,undefined")
