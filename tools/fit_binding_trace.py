"""What every host form of a Fitter hands to the library, without a GPU and without the library: runs
tests/fit_binding_calls.py's list of calls on a fitter with a recording stand-in and prints, per call, the export's name, every
argument (its ctypes kind and value; the dtype, shape and a digest of the array behind a pointer) and what the call returned.  The
output names no address, so that of two trees can be compared with diff: `--tree` is the root of the other one (its depthhead_amd
is imported in place of this one's).  `--time N` prints instead the median time of N calls of each case, in microseconds: the cost
of binding the arguments alone, since the stand-in does nothing."""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--time", type=int, default=0)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import fit_binding_calls as fb
    from depthhead_amd import _lib, fit
    rec = fb.Recorder()
    f = fb.fitter(fit, rec)
    cases = fb.host_cases(fit, _lib)
    if a.time:
        kinds = {}
        for label, call in cases:
            t = []
            for _ in range(a.time):
                t0 = time.perf_counter()
                call(f)
                t.append(time.perf_counter() - t0)
                rec.calls.clear()
            kinds.setdefault(label.split()[0], []).append(1e6 * float(np.median(t)))
            print("%-40s %8.2f us" % (label, 1e6 * float(np.median(t))))
        for kind, us in kinds.items():
            print("kind %-35s %8.2f us (median of its %d cases)" % (kind, float(np.median(us)), len(us)))
        return
    traced = fb.TracingNumpy()
    fit.np = _lib.np = traced
    for label, call in cases:
        out = call(f)
        (name, args), = rec.calls
        rec.calls.clear()
        print(f"{label}: {name}")
        for i, arg in enumerate(args):
            print(f"  {i}: {fb.describe(arg, traced.made)}")
        print(f"  -> {fb.result(out)}")
    print(f"{len(cases)} calls")


if __name__ == "__main__":
    main()
