#!/usr/bin/env python3
"""Record tests/golden/abi_refusals.json: the (status, message) every case of
tests/abi_refusal_cases.py gets from the built library, keyed by entry point and case name.
Needs an MI355X.  Run it against the library whose behaviour is to be pinned (the commit BEFORE a
change of rajepy_amd/csrc/rjprt.hip), commit the file, and leave it alone afterwards:
tests/test_gpu_refusals.py holds every later library to it.

    python tools/record_abi_refusals.py [--out FILE]

A case the library ACCEPTS ends the run at once: the table is meant to hold refusals only."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "abi_refusals.json"))
    args = ap.parse_args()
    from rajepy_amd import _lib
    from rajepy_amd.engine import RTEngine
    from tests import abi_refusal_cases as T
    eng = RTEngine(0)
    env = T.Env(eng)
    eng.synchronize()
    out = {}
    for name in T.ENTRIES:
        rec = out[name] = {}
        for case, change in T.cases(name):
            status, msg = T.call(env, name, change)
            if status >= _lib.RJP_OK:
                sys.exit("%s / %s was accepted (status %d): not a refusal" % (name, case, status))
            rec[case] = [status, msg]
        status, _ = T.call(env, name)
        eng.synchronize()
        if status != _lib.RJP_OK:
            sys.exit("%s: the valid call failed (status %d): %s"
                     % (name, status, eng.lib.rjp_last_error(eng.ctx).decode()))
    eng.close()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d entry points, %d cases -> %s" % (len(out), sum(len(v) for v in out.values()),
                                               args.out))


if __name__ == "__main__":
    main()
