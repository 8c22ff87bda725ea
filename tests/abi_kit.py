"""What the ABI tests share (tests/test_abi*.py): the last error, the public header's text and the names it
declares, the block "exported, declared, through the guard" every family repeats, the g++ program that prints a struct's layout,
and the ctypes stand-ins for handles that live on a device.  The refusal tests themselves are the files' own."""
import ctypes as C
import os
import re

import host_program
import runtime_units
from depthhead_amd import _lib

INCLUDE = os.path.join(host_program.ROOT, "include")


def err(lib):
    return lib.dh_last_error().decode()


def header():
    """The text of include/depthhead_hip.h."""
    return open(os.path.join(INCLUDE, "depthhead_hip.h")).read()


def declared():
    """The dh_ names the header declares."""
    return set(re.findall(r"^(?:int|const char \*)\s*(dh_\w+)\(", header(), re.M))


def declared_args(name):
    """The argument list of `name`'s declaration, each argument with its white space normalised."""
    return [" ".join(a.split()) for a in re.search(r"int %s\((.*?)\);" % name, header(), re.S).group(1).split(",")]


def assert_exported(lib, names):
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n), n


def assert_header_equals_exports(names, *phrases):
    """Each of `names` is declared and generated through the exception guard, the header declares the export list and nothing else,
    and says each of `phrases`."""
    text, api = header(), runtime_units.text()
    for n in names:
        assert f"int {n}(" in text, n
        assert f"DH_API({n[3:]}," in api, n
    assert declared() == set(_lib.EXPORTS), declared() ^ set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    for p in phrases:
        assert p in text, p


def layouts(tmp_path, cpp_text):
    """Compiles `cpp_text` against the header and runs it.  It prints "<struct> size <n>", "<struct> <field> <offset>" and at most
    one line "consts <value> ...": ({(struct, field or "size"): number}, the consts' words as printed)."""
    src = tmp_path / "layout.cpp"
    src.write_text(cpp_text)
    out = host_program.run(host_program.build(tmp_path, "layout", [src], extra=("-I" + INCLUDE,)), timeout=60).stdout.split("\n")
    c = {tuple(line.split()[:2]): int(line.split()[2]) for line in out if line and not line.startswith("consts")}
    consts = [w for line in out if line.startswith("consts") for w in line.split()[1:]]
    return c, consts


# Handles live on a device, so where a refusal is decided before a handle's device memory is used the calls get a block that reads
# as one: the struct's leading fields, then zeros up to a size no smaller than the struct's.
class Cameras(C.Structure):
    """dh_cameras (dh_runtime.h): device, n."""
    _fields_ = [("device", C.c_int), ("n", C.c_int), ("rest", C.c_uint8 * 248)]


class Views(C.Structure):
    """dh_fit_views (dh_runtime_fit.h): device, n, the camera table it is bound to."""
    _fields_ = [("device", C.c_int), ("n", C.c_int), ("cams", C.c_void_p), ("rest", C.c_uint8 * 240)]


class Model(C.Structure):
    """dh_fit_model (dh_runtime_fit.h): device, n, radius."""
    _fields_ = [("device", C.c_int), ("n", C.c_uint32), ("radius", C.c_double), ("rest", C.c_uint8 * 240)]


class Basis(C.Structure):
    """dh_fit_basis (dh_api_fit.hip): device, n, k, (padding), largest."""
    _fields_ = [("device", C.c_int), ("n", C.c_uint32), ("k", C.c_uint32), ("pad", C.c_uint32), ("largest", C.c_double), ("rest", C.c_uint8 * 232)]


class SubjectSet(C.Structure):
    """dh_fit_subjects (dh_api_fit.hip): device, n, n_tris, n_subjects, max_coeff, radius, its basis."""
    _fields_ = [("device", C.c_int), ("n", C.c_uint32), ("n_tris", C.c_uint32), ("n_subjects", C.c_uint32), ("max_coeff", C.c_double),
                ("radius", C.c_double), ("basis", C.c_void_p), ("rest", C.c_uint8 * 472)]
