"""The host side of a surface set that is plain functions (depthhead_amd/csrc/dh_fit.h) -- the neighbour lists
dh_fit_subjects_create_surface builds and the grown radius bound -- checked by tests/host/surface_check.cpp, a stand-alone program
with its own main: built by plain g++ once as it is and once with -fsanitize=address,undefined, and run, by
tests/host_program.py.  Nothing of HIP is linked or run, and nothing is loaded into Python.  No GPU."""
import host_program as hp


def check(tmp_path, sanitize=None):
    exe = hp.build(tmp_path, "surface_check", [hp.host("surface_check.cpp")], sanitize, hp.fit_header_flags())
    hp.run(exe, min_ok=2000, timeout=300)


def test_neighbour_lists_and_the_grown_radius_bound_on_the_host(tmp_path):
    check(tmp_path)


def test_the_same_under_asan_ubsan(tmp_path):
    check(tmp_path, "address,undefined")
