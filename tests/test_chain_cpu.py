"""The swap chain's shared slot (include/crender_chain.h, csrc/chain.hip): what can be checked without a GPU —
the header against the library's exports and the ctypes table, the unit's place in the build, and the argument
errors that return before anything touches the HIP runtime."""
import ctypes as C
import os
import re
import subprocess

from pass_scenes import capi  # noqa: F401 (fixtures)
from util import INCLUDE, other_symbols, unit_in_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_header_symbols_are_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_chain.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["chain"])
    assert {"crender_pipeline_share_stream", "crender_pipeline_unshare", "crender_pipeline_shared_slot"} <= declared
    assert not declared & other_symbols(capi, "chain")
    L = capi.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    kind = {"crender_pipeline *": C.c_void_p, "const crender_pipeline *": C.c_void_p, "void *": C.c_void_p, "int ": C.c_int}
    for name in declared:
        res, args = capi.UNIT_SIGNATURES["chain"][name]
        fn = getattr(L, name)
        assert fn.restype == res == C.c_int and fn.argtypes == args, name
        # every parameter of the declaration, by its type, against the table
        decl = re.search(r"CRENDER_API int " + name + r"\((.*?)\);", header, re.S).group(1)
        want = [kind[re.match(r"\s*(.*?)\w+$", a).group(1)] for a in decl.split(",")]
        assert want == args, name
    assert capi.UNIT_SIGNATURES["chain"]["crender_pipeline_share_stream"][1] == [C.c_void_p, C.c_int, C.c_void_p]
    assert capi.ABI_VERSION == 6


def test_chain_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit_in_build(_build, "chain", ["chain.hip"], [os.path.join(INCLUDE, "crender_chain.h")])
    # host code over the pipeline handle of plan.h: no kernel, no launch
    unit = open(os.path.join(_build.SRC_DIR, "chain.hip")).read()
    assert '#include "plan.h"' in unit
    assert "__global__" not in unit and "<<<" not in unit and "hipLaunchKernelGGL" not in unit


def test_chain_argument_errors_without_a_gpu(capi):
    L = capi.load()
    assert L.crender_pipeline_share_stream(None, 0, None) == capi.EINVAL
    assert b"null pipeline" in L.crender_last_error()
    assert L.crender_pipeline_unshare(None) == capi.EINVAL
    assert b"crender_pipeline_unshare" in L.crender_last_error()
    assert L.crender_pipeline_shared_slot(None) == -1
    assert L.crender_pipeline_owned_streams(None) == -1


def test_the_package_sets_no_runtime_variable():
    """The depth rule READS GPU_MAX_HW_QUEUES; nothing in the package writes the environment."""
    pkg = os.path.join(ROOT, "cython3dmodelrenderer_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                assert not re.search(r"os\.environ\s*\[[^\]]*\]\s*=|environ\.setdefault|os\.putenv", text), f
