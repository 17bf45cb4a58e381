"""Fixture of tests/test_renderer_protocol_cpu.py: tests/golden/renderer_protocol.json, what the Renderer asks of its
fillers (or the refusal) for every ``on_device``, three kinds of illumination and every option alone and in pairs.

The cases and the recording are the test's own (tests/test_renderer_protocol_cpu.py: cases, outcomes, packed); the
Renderer is the one to record FROM: cython3dmodelrenderer_amd/renderer.py of the commit before its option checks and
its frame sequence were folded, put in place of the current one
(`git show THAT_COMMIT:cython3dmodelrenderer_amd/renderer.py > cython3dmodelrenderer_amd/renderer.py`).  The output
holds no address and no time: two runs over the same renderer.py write the same bytes.  Needs no GPU and no library.

usage: python scripts/make_renderer_protocol_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    if len(sys.argv) != 1:
        sys.exit(__doc__)
    import test_renderer_protocol_cpu as cases
    got = cases.outcomes()
    doc = cases.packed(got)
    raises = sum("raises" in o for o in got.values())
    print(len(got), "cases:", len(got) - raises, "render,", raises, "raise;", len(doc["outcomes"]), "outcomes,",
          len(doc["calls"]), "calls")
    # one call, one case and one outcome per line, without spaces: the file stays small and a change shows as its lines
    line = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))        # noqa: E731
    with open(cases.FIXTURE, "w") as fh:
        fh.write('{"calls":[\n' + ",\n".join(line(c) for c in doc["calls"]))
        fh.write('],\n"cases":{\n' + ",\n".join(f"{line(k)}:{i}" for k, i in sorted(doc["cases"].items())))
        fh.write('},\n"outcomes":[\n' + ",\n".join(line(o) for o in doc["outcomes"]) + "]}\n")


if __name__ == "__main__":
    main()
