"""Fixture of tests/test_pass_arg_order_cpu.py: tests/golden/pass_arg_order.json, the return code and the text of
crender_last_error() for every single bad argument and every pair of them that the test makes, per entry.

The cases are the test's own (tests/test_pass_arg_order_cpu.py: entries, outcomes); the library is the one to record
FROM: a build of the commit before the entries' frame checks were shared (its libcrender_hip.so, built with
`python -m cython3dmodelrenderer_amd._build` in a checkout of that commit).  Needs no GPU: every call fails its checks.

usage: python scripts/make_pass_arg_order_golden.py PATH_TO_THAT_LIBRARY
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        sys.exit(__doc__)
    os.environ["CRENDER_LIB"] = os.path.abspath(sys.argv[1])      # _capi.lib_path()
    from cython3dmodelrenderer_amd import _capi
    import test_pass_arg_order_cpu as cases
    doc = {}
    for entry, got in cases.outcomes(_capi).items():
        # the few distinct (return code, text) once, and each case's place among them
        distinct = sorted({tuple(v) for v in got.values()})
        doc[entry] = {"outcomes": [list(v) for v in distinct], "cases": {k: distinct.index(tuple(v)) for k, v in got.items()}}
        print(entry, len(got), "cases,", len(distinct), "outcomes")
    with open(cases.FIXTURE, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
