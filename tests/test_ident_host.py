"""The decision of an identification that is plain functions of depthhead_amd/csrc/dh_fit.h -- the order, the
status, the mean square and the picks the decide wave keeps and merges -- checked by tests/host/ident_check.cpp, a stand-alone
program with its own main: built by plain g++ once as it is and once with -fsanitize=address,undefined, and run, by
tests/host_program.py.  The kernel compiles the very same functions.  Nothing of HIP is linked or run, and
nothing is loaded into Python.  No GPU."""
import host_program as hp


def check(tmp_path, sanitize=None):
    exe = hp.build(tmp_path, "ident_check", [hp.host("ident_check.cpp")], sanitize, hp.fit_header_flags())
    hp.run(exe, min_ok=10000, timeout=300)


def test_the_order_the_status_and_the_picks_against_a_sort(tmp_path):
    check(tmp_path)


def test_the_same_under_asan_ubsan(tmp_path):
    check(tmp_path, "address,undefined")
