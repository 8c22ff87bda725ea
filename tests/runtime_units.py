"""The host runtime's sources as text, for the tests that read the ABI off them (every export through the exception guard).  The
runtime is being cut into one translation unit per family of entry points; the list of units comes from
build.SOURCES -- every .hip source that is not a kernel unit (k_*.hip) -- so a unit added later is read without touching a test.
The runtime's internal headers are those of build.HEADERS named dh_runtime*.h: a header that defines a DH_API macro or an entry
point must carry that name, or these tests do not see it."""
import os
import re

from depthhead_amd import build

UNITS = [s for s in build.SOURCES if s.endswith(".hip") and not s.startswith("k_")]
HEADERS = [h for h in build.HEADERS if h.startswith("dh_runtime")]


def read(name):
    """The text of one source of the library."""
    return open(os.path.join(build.CSRC, name)).read()


def units():
    """{file name: text} of every runtime unit."""
    return {u: read(u) for u in UNITS}


def headers():
    """{file name: text} of the runtime's internal headers."""
    return {h: read(h) for h in HEADERS}


def text():
    """Every runtime unit, one after the other."""
    return "\n".join(units().values())


def guarded():
    """The exports the units generate through the guard: one DH_API line each."""
    return set("dh_" + m for m in re.findall(r"^DH_API\((\w+),", text(), flags=re.M))


def raw_definitions(src):
    """The extern "C" functions `src` defines by hand."""
    return set(re.findall(r'extern "C" (?:int|const char \*)\s*(dh_\w+)\(', src))


def api_macros():
    """{macro name: body} of every DH_API* macro the runtime's sources define, continuation lines included."""
    found = re.findall(r"^#define (DH_API\w*)\([^)]*\)((?:.*\\\n)*.*)$", "\n".join(list(headers().values()) + [text()]), flags=re.M)
    assert len(found) == len(set(n for n, _ in found)), found        # (each defined once: no unit brings its own)
    return dict(found)
