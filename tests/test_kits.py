"""The helper modules the tests share -- gpu_kit's record compare and guard bands on host arrays, host_program
on throw-away programs written here, abi_kit's reading of the header -- checked for the failures they exist to report.  Every
program has its own main and is run as a process of its own.  No GPU."""
import re

import numpy as np
import pytest

import abi_kit
import gpu_kit
import host_program as hp
from depthhead_amd import _lib

REC = np.dtype([("id", "<u4"), ("t", "<f4", (3,))])


def records(n, dtype=REC):
    a = np.zeros(n, dtype)
    a.view(np.uint8)[:] = np.arange(a.nbytes) % 251
    return a


def test_same_records_passes_on_equal_arrays_and_names_what_differs():
    want = records(5)
    gpu_kit.same_records(want.copy(), want, "equal")
    gpu_kit.same_records(want.copy().reshape(5, 1), want, "equal, another shape")
    last_byte = want.copy()
    last_byte.view(np.uint8)[-1] ^= 1
    wider = np.zeros(5, np.dtype(REC.descr + [("pad", "<u4")]))
    for name, got in (("last byte", last_byte), ("shorter", want[:4]), ("longer", records(6)), ("item size", wider)):
        with pytest.raises(AssertionError, match=name):
            gpu_kit.same_records(got, want, name)


def test_untouched_sees_one_byte_in_either_band():
    off, nbytes = gpu_kit.GUARD + 8, 100
    buf = np.full(off + nbytes + gpu_kit.GUARD, gpu_kit.FILL, np.uint8)
    buf[off:off + nbytes] = 7                                    # only the payload changed
    assert gpu_kit.untouched(buf, off, nbytes)
    for at in (0, off - 1, off + nbytes, len(buf) - 1):
        bad = buf.copy()
        bad[at] ^= 1
        assert not gpu_kit.untouched(bad, off, nbytes), at


def program(tmp_path, body, name="prog", sanitize=None):
    src = tmp_path / (name + ".cpp")
    src.write_text("#include <limits.h>\n#include <stdio.h>\nint main(int argc, char **argv) { %s }\n" % body)
    return hp.build(tmp_path, name, [src], sanitize, hp.WARN)


def test_run_requires_a_count_above_min_ok_and_exit_status_zero(tmp_path):
    ok5 = program(tmp_path, 'printf("ok 5\\n"); return 0;', "ok5")
    assert hp.run(ok5, min_ok=4, timeout=60).stdout == "ok 5\n"
    with pytest.raises(AssertionError):
        hp.run(ok5, min_ok=5, timeout=60)
    with pytest.raises(AssertionError):
        hp.run(program(tmp_path, 'printf("done 9\\n"); return 0;', "no_ok"), min_ok=4, timeout=60)
    with pytest.raises(AssertionError):
        hp.run(program(tmp_path, 'printf("ok 5\\n"); return 1;', "exit1"), timeout=60)
    echo = program(tmp_path, 'char s[16] = ""; if (scanf("%15s", s) != 1) return 2; printf("%s %s\\n", argv[argc - 1], s); return 0;', "echo")
    assert hp.run(echo, stdin="in", args=(7,), timeout=60).stdout == "7 in\n"
    assert hp.run(echo, stdin=b"in", args=("x",), timeout=60).stdout == b"x in\n"


def test_a_program_that_does_not_build_fails(tmp_path):
    """Whatever the compiler's message says: a skip is decided before the program under test is built."""
    with pytest.raises(AssertionError, match="unrecognized"):
        program(tmp_path, "return unrecognized;", "broken", sanitize="undefined")


def test_the_sanitizer_flags_reach_the_compiler(tmp_path):
    """INT_MAX + argc overflows a signed int: under -fsanitize=undefined (not recovered) the program ends non-zero, without it zero."""
    body = 'int x = INT_MAX; x += argc; printf("ok %d\\n", x < 0); return 0;'
    hp.run(program(tmp_path, body, "plain"), timeout=60)
    with pytest.raises(AssertionError, match="signed integer overflow"):
        hp.run(program(tmp_path, body, "checked", sanitize="undefined"), timeout=60)


def test_the_header_declares_the_export_list_whichever_expression_reads_it():
    text = abi_kit.header()
    assert abi_kit.declared() == set(_lib.EXPORTS) and len(abi_kit.declared()) == len(_lib.EXPORTS)
    # the expression one ABI file used before they shared abi_kit.declared()
    assert set(re.findall(r"^(?:int|const char \*)\s*(dh_[a-z0-9_]+)\(", text, re.M)) == abi_kit.declared()
    assert abi_kit.declared_args("dh_version") == ["void"]
    assert abi_kit.declared_args("dh_fit_calibrate_views_device")[-1] == "void *stream"
