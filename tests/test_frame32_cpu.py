"""The small-scene frame kernel (include/crender_frame32.h, csrc/frame32.hip): what can be checked without a GPU —
the unit's place in the build, outside the profile fingerprint; the header against the library's exports and the
ctypes table; the argument errors that return before anything touches the HIP runtime; the filler's switch.

The unit sits in ``_build.FRAME_UNITS`` / ``_capi.FRAME_SIGNATURES`` and is linked through ``_build.link_sources()``:
``_build.UNITS``, ``_build.library_sources()``, ``_build.build_inputs()`` and ``_capi.UNIT_SIGNATURES`` are pinned name for name by the feature
units' tests (test_host_cpu, test_wire_pass_cpu, test_edge_aa_cpu, ...), so they stay as they are — checked below."""
import ctypes as C
import os
import re
import subprocess

from pass_scenes import capi  # noqa: F401 (fixtures)
from util import other_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    header = open(os.path.join(ROOT, "include", "crender_frame32.h")).read()
    return header, set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))


def test_frame32_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    sources, headers = _build.FRAME_UNITS["frame32"]
    assert list(_build.FRAME_UNITS) == list(__import__("cython3dmodelrenderer_amd._capi", fromlist=["x"]).FRAME_SIGNATURES)
    assert sources == ["frame32.hip"]
    assert len(headers) == 1 and headers[0].endswith("crender_frame32.h")
    for name in sources + headers:
        assert os.path.exists(os.path.join(_build.SRC_DIR, name)), name
    # the default build compiles the unit, and a change of it makes the library stale
    assert _build.link_sources() == _build.library_sources() + sources
    assert set(_build.frame_inputs()) == {os.path.join(_build.SRC_DIR, name) for name in sources + headers}
    # ... and the tables the other units' tests pin are untouched
    assert "frame32" not in _build.UNITS and "frame32.hip" not in _build.library_sources()
    assert not set(_build.frame_inputs()) & set(_build.build_inputs())
    # none of it is fingerprinted, and the fingerprint is the one the committed profiles were measured on
    fingerprinted = _build.SOURCES + _build.HEADERS
    assert not set(sources + headers) & set(fingerprinted)
    assert not any("frame32" in name for name in fingerprinted)
    assert _build.source_sha16() == "35a9bf480abfca1e"
    # the kernel's arithmetic is the shared headers', and the binning wavefronts are binning.h's
    unit = open(os.path.join(_build.SRC_DIR, "frame32.hip")).read()
    assert '#include "plan.h"' in unit and "setup_wave_body<TS, true>" in unit
    for fn in ("make_setup", "numerators", "fragment_from", "quotients", "shade_and_store", "store_background"):
        assert re.search(r"\b" + fn + r"\b", unit), fn
    assert not re.search(r"#include\s+\"[^\"]*\.hip\"", unit)


def test_the_library_is_stale_when_the_frame_kernel_is_newer(tmp_path, monkeypatch):
    from cython3dmodelrenderer_amd import _build
    lib = tmp_path / "libcrender_hip.so"
    monkeypatch.setattr(_build, "LIB_PATH", str(lib))
    lib.write_bytes(b"")
    newest = max(os.path.getmtime(path) for path in _build.frame_inputs())
    os.utime(lib, (newest + 1, newest + 1))
    assert not _build.needs_build(_build.frame_inputs())
    for path in _build.frame_inputs():
        then = os.path.getmtime(path) - 1
        os.utime(lib, (then, then))
        assert _build.needs_build(_build.frame_inputs()), path
    built = []
    monkeypatch.setattr(_build, "compile_library", lambda out, **kw: built.append(out) or out)
    monkeypatch.setattr(_build, "build_inputs", lambda: [])
    assert _build.build() == str(lib) and built == [str(lib)]         # build() counts the frame kernels' files


def test_frame32_header_symbols_are_exported_and_bound(capi):
    header, declared = _declared()
    assert declared == set(capi.FRAME_SIGNATURES["frame32"]) == {"crender_frame32_submit", "crender_frame32_last"}
    assert "frame32" not in capi.UNIT_SIGNATURES and not declared & other_symbols(capi, "frame32")
    L = capi.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    kind = {"crender_pipeline *": C.c_void_p, "const crender_pipeline *": C.c_void_p, "void *": C.c_void_p}
    for name in declared:
        res, args = capi.FRAME_SIGNATURES["frame32"][name]
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
