"""The two plain functions of a multi-view shape step (depthhead_amd/csrc/dh_fit.h) -- dh_shape_view_bit,
the r-th set bit of a view mask, and dh_shape_views_skip, the whole-instance test of the host loop and of
k_shape_accumulate_views -- checked on the host by tests/host/shape_views_check.cpp, a stand-alone program with its own main:
built by plain g++ once as it is and once with -fsanitize=address,undefined, and run.  dh_fit.h declares the kernels' launchers,
so the HIP headers are on the include path (beside the hipcc that build() uses); nothing of HIP is linked or run, and nothing is
loaded into Python.  No GPU."""
import host_program as hp


def check(tmp_path, sanitize=None):
    exe = hp.build(tmp_path, "shape_views_check", [hp.host("shape_views_check.cpp")], sanitize, hp.fit_header_flags())
    hp.run(exe, min_ok=400 * 66, timeout=300)


def test_the_rank_selection_and_the_skip_test_on_the_host(tmp_path):
    check(tmp_path)


def test_the_same_under_asan_ubsan(tmp_path):
    check(tmp_path, "address,undefined")
