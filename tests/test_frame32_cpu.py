"""The small-scene frame kernel (include/crender_frame32.h, csrc/frame32.hip): what can be checked without a GPU —
the unit's place in the build, outside the profile fingerprint; the header against the library's exports and the
ctypes table; the argument errors that return before anything touches the HIP runtime; the filler's switch."""
import ctypes as C
import os
import re
import subprocess

from pass_scenes import capi  # noqa: F401 (fixtures)
from util import INCLUDE, other_symbols, unit_in_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    header = open(os.path.join(ROOT, "include", "crender_frame32.h")).read()
    return header, set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))


def test_frame32_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit_in_build(_build, "frame32", ["frame32.hip"], [os.path.join(INCLUDE, "crender_frame32.h")])
    # the kernel's arithmetic is the shared headers', and the binning wavefronts are binning.h's
    unit = open(os.path.join(_build.SRC_DIR, "frame32.hip")).read()
    assert '#include "plan.h"' in unit and "setup_wave_body<TS, true>" in unit
    for fn in ("make_setup", "numerators", "fragment_from", "quotients", "shade_and_store", "store_background"):
        assert re.search(r"\b" + fn + r"\b", unit), fn
    assert not re.search(r"#include\s+\"[^\"]*\.hip\"", unit)


def test_frame32_header_symbols_are_exported_and_bound(capi):
    header, declared = _declared()
    assert declared == set(capi.UNIT_SIGNATURES["frame32"]) == {"crender_frame32_submit", "crender_frame32_last"}
    assert not declared & other_symbols(capi, "frame32")
    L = capi.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    kind = {"crender_pipeline *": C.c_void_p, "const crender_pipeline *": C.c_void_p, "void *": C.c_void_p}
    for name in declared:
        res, args = capi.UNIT_SIGNATURES["frame32"][name]
        fn = getattr(L, name)
        assert fn.restype == res == C.c_int and fn.argtypes == args, name
        decl = re.search(r"CRENDER_API int " + name + r"\((.*?)\);", header, re.S).group(1)
        assert [kind[re.match(r"\s*(.*?)\w+$", a).group(1)] for a in decl.split(",")] == args, name


def test_frame32_argument_errors_without_a_gpu(capi):
    L = capi.load()
    assert L.crender_frame32_submit(None, None) == capi.EINVAL
    assert b"null pipeline" in L.crender_last_error()
    assert L.crender_frame32_last(None) == 0


def test_the_filler_has_the_switch_and_the_extension_both_entries():
    import inspect
    from cython3dmodelrenderer_amd.pixel_buffer_filler import advanced_pixel_buffer_filler as mod
    sig = inspect.signature(mod.AdvancedPixelBufferFiller.__init__)
    assert sig.parameters["frame32"].default is None and sig.parameters["frame32"].kind is inspect.Parameter.KEYWORD_ONLY
    assert isinstance(mod._FRAME32_DEFAULT, bool)
    ext = open(os.path.join(ROOT, "cython3dmodelrenderer_amd", "csrc", "crender_torch.cpp")).read()
    assert re.search(r"void pipeline_submit\(.*?crender_frame32_submit\(", ext, re.S)
    assert re.search(r"void pipeline_submit_general\(.*?crender_pipeline_submit\(", ext, re.S)
