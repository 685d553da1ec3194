#!/usr/bin/env python3
"""OFDM_MI355X_LIB=<library of the PARENT commit> python tests/golden/gen_despread_refusals.py [out.json]

Records tests/golden/despread_refusals.json: status and ofdm_last_error() text of every case of tests/despread_refusal_cases.py in
every handle state it runs in, made on a library built from the commit IN FRONT OF the change under test (needs a GPU for the two
handles; no case launches a kernel).  Refuses to run on the tree's own library, so that a change can never record its own
behaviour as the expectation."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "lte-gnu-radio-code_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    lib = os.environ.get("OFDM_MI355X_LIB")
    if not lib or not os.path.exists(lib):
        sys.exit("set OFDM_MI355X_LIB to a library built from the parent commit")
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    own = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "libofdm_mi355x.so")
    if os.path.exists(own) and os.path.samefile(lib, own):
        sys.exit("OFDM_MI355X_LIB is this tree's own library: record from a build of the parent commit")
    import despread_refusal_cases as cases
    ofdm_mi355x.load()
    out = cases.Runner(ofdm_mi355x).run_all()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "despread_refusals.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    each = [v for of in out.values() for v in of.values()]
    flat = [r for v in each for r in (v.values() if isinstance(v, dict) else [v])]
    print("%d cases, %d of them differ between the handle states, %d distinct texts -> %s"
          % (len(each), sum(isinstance(v, dict) for v in each), len({r[1] for r in flat}), path))


if __name__ == "__main__":
    main()
