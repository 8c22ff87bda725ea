"""The binding lifecycle and the bind-or-retry update of the subject trackers (DESIGN.md sections 29 and 30) that are plain functions
of depthhead_amd/csrc/dh_fit.h -- dh_subject_lifecycle, dh_subject_bind_or_retry, dh_subject_unbind, dh_sat_inc -- and the decision
over a row of multi-view scores, checked by tests/host/subject_bind_check.cpp, a stand-alone program with its own main: built by
plain g++ once as it is and once with -fsanitize=address,undefined, and run, by tests/host_program.py.
The kernels compile the very same functions.  Nothing of HIP is linked or run, and nothing is loaded into Python.  No GPU."""
import host_program as hp


def check(tmp_path, sanitize=None):
    exe = hp.build(tmp_path, "subject_bind_check", [hp.host("subject_bind_check.cpp")], sanitize, hp.fit_header_flags())
    hp.run(exe, min_ok=50000, timeout=300)


def test_the_lifecycle_and_the_decision_against_the_headers_text(tmp_path):
    check(tmp_path)


def test_the_same_under_asan_ubsan(tmp_path):
    check(tmp_path, "address,undefined")
