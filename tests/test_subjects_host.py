"""The host side of a subject set that is plain functions (depthhead_amd/csrc/dh_fit.h) -- the corner lists
dh_fit_subjects_create builds, the base mesh's zero-normal test and the radius bound -- checked by tests/host/subjects_check.cpp, a
stand-alone program with its own main: built by plain g++ once as it is and once with -fsanitize=address,undefined, and run, by
tests/host_program.py (the sanitizer's presence is probed with a trivial program first).  Nothing of HIP is linked or run, and nothing is loaded into Python.  No GPU."""
import host_program as hp


def check(tmp_path, sanitize=None):
    exe = hp.build(tmp_path, "subjects_check", [hp.host("subjects_check.cpp")], sanitize, hp.fit_header_flags())
    hp.run(exe, min_ok=2000, timeout=300)


def test_corner_lists_zero_normals_and_the_radius_bound_on_the_host(tmp_path):
    check(tmp_path)


def test_the_same_under_asan_ubsan(tmp_path):
    check(tmp_path, "address,undefined")
