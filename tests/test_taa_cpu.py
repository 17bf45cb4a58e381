"""Temporal anti-aliasing without a GPU: the header against the binding and the library, the unit's provisional place in
the build, the entry point's argument checks, the host model the GPU tests compare with (tests/taa_ref.py) pinned by
hand-made planes and against its own float64 evaluation, the convergence of a still T-Rex towards the supersampled image and
the orderings under motion (frames by the oracle), ``AdvancedPixelBufferFiller.temporal_resolve``'s protocol on CPU tensors
and ``Renderer(temporal_aa=...)``."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import motion_ref
import taa_ref
from pass_scenes import LIGHT, Frame, capi, fake_filler_base, recording_filler, soups_fixture, trex_arrays  # noqa: F401 (fixtures)
from util import LIBRARY_SOURCES, UNIT_KEYS, assert_bit_equal, other_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOLVE, VECTORS = "crender_taa_resolve", "crender_motion_vectors"
_vp, _i32 = C.c_void_p, C.c_int
ARGTYPES = [_vp, _vp, _vp, _vp, C.c_float, _vp, _i32, _i32, _i32, _i32, C.c_uint, _vp]
NAN, INF = np.float32(np.nan), np.float32(np.inf)


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_taa_symbol_is_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_taa.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.PENDING["taa"]) == {RESOLVE} and list(capi.PENDING) == ["taa"]
    assert not declared & other_symbols(capi, None)               # the core ABI's and every unit's
    L = capi.load()
    res, args = capi.PENDING["taa"][RESOLVE]
    assert res == C.c_int and args == ARGTYPES == getattr(L, RESOLVE).argtypes
    decl = [" ".join(a.split()) for a in re.search(r"CRENDER_API int " + RESOLVE + r"\((.*?)\);", header, re.S).group(1).split(",")]
    assert decl == ["const float *d_color", "const float *d_history", "const float *d_velocity", "const float *d_z",
                    "float blend", "float *d_out", "int H", "int W", "int y0", "int y1", "unsigned flags", "void *stream"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert RESOLVE in set(re.findall(r" T (crender_\w+)", out))
    assert int(re.search(r"#define CRENDER_TAA_NO_CLAMP (\d+)u", header).group(1)) == capi.TAA_NO_CLAMP == taa_ref.NO_CLAMP == 1
    assert "CRENDER_ABI_VERSION" in header and capi.ABI_VERSION == 6          # the change is additive, and the header says so
    # 3 to 6 planes of the staged tile stay far below 64 KB: no launch attribute
    assert (3 * 34 * 34 * 4, 6 * 34 * 34 * 4) == (13872, 27744)


def test_taa_unit_is_linked_from_the_pending_table_and_stays_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    assert list(_build.PENDING) == ["taa"]
    assert _build.PENDING["taa"] == (["temporal.hip"], [os.path.join("..", "..", "include", "crender_taa.h")])
    # the pinned tables are what they were
    assert list(_build.UNITS) == UNIT_KEYS and _build.library_sources() == LIBRARY_SOURCES
    assert _build.source_sha16() == "35a9bf480abfca1e"
    assert not {"temporal.hip", "crender_taa.h"} & {os.path.basename(n) for n in _build.SOURCES + _build.HEADERS}
    assert _build.pending_sources() == ["temporal.hip"]
    pending = _build.pending_inputs()
    assert len(pending) == 2 and all(os.path.isfile(p) for p in pending) and not set(pending) & set(_build.build_inputs())
    # the default build links the pending sources behind the library's
    default = inspect.signature(_build.compile_library).parameters["sources"].default
    assert default is None and "library_sources() + pending_sources()" in inspect.getsource(_build.compile_library)
    text = open(os.path.join(_build.SRC_DIR, "temporal.hip")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<math.h>", '"common.h"', '"../../include/crender_taa.h"', '"winner_pass.h"']
    assert text.count("namespace {") == 1 and text.count('extern "C" {') == 1 and "asm" not in text
    body = text[text.index("void k_taa_resolve"):text.index("}  // namespace")]
    assert "extern __shared__" in body and body.count("__syncthreads()") == 2 and "wave_any(" in body
    code = "".join(line.split("//")[0] for line in body.splitlines())
    assert "sqrtf" not in code and "float)" in code and " / (" not in code         # no root and no float quotient
    from cython3dmodelrenderer_amd import _capi
    assert "PENDING.values()" in inspect.getsource(_capi.load)


def test_a_newer_pending_input_makes_build_rebuild(tmp_path, monkeypatch):
    from cython3dmodelrenderer_amd import _build
    lib = tmp_path / "libcrender_hip.so"
    monkeypatch.setattr(_build, "LIB_PATH", str(lib))
    built = []
    monkeypatch.setattr(_build, "compile_library", lambda out, **kw: built.append(out) or out)
    lib.write_bytes(b"")
    everything = _build.build_inputs() + _build.pending_inputs()
    newest = max(os.path.getmtime(path) for path in everything)
    os.utime(lib, (newest + 1, newest + 1))
    assert not _build.needs_build() and not _build.needs_build(_build.pending_inputs())
    assert _build.build() == str(lib) and built == []
    for path in _build.pending_inputs():
        then = os.path.getmtime(path) - 1
        os.utime(lib, (then, then))
        assert _build.needs_build(_build.pending_inputs()), path
        assert _build.build() == str(lib) and built == [str(lib)], path
        built.clear()
    # needs_build() without arguments keeps its meaning: the pinned inputs alone
    newest = max(os.path.getmtime(path) for path in _build.build_inputs())
    oldest_pending = min(os.path.getmtime(path) for path in _build.pending_inputs())
    if oldest_pending > newest:
        os.utime(lib, (newest + 0.5, newest + 0.5))
        assert not _build.needs_build()


def test_taa_resolve_argument_errors_without_a_gpu(capi):
    L, E = capi.load(), capi.EINVAL
    col, hist, out, vel, z = (C.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))   # never dereferenced
    nan, inf = float("nan"), float("inf")

    def call(col=col, hist=hist, vel=vel, z=z, blend=0.1, out=out, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_taa_resolve(col, hist, vel, z, blend, out, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(col=None), dict(hist=None), dict(out=None)):
        assert call(**kw) == E and "d_color, d_history or d_out is NULL" in text(), kw
    assert call(vel=None) == E and "d_z without d_velocity" in text()
    for kw in (dict(H=0), dict(W=-2), dict(H=-2 ** 31)):
        assert call(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert call(**kw) == E and "rows outside the frame" in text(), kw
    for flags in (2, 3, 0x80000000):
        assert call(flags=flags) == E and "unknown flag bits" in text(), flags
    for kw in (dict(out=col), dict(out=hist)):
        assert call(**kw) == E and "d_out is d_color or d_history" in text(), kw
    for bad in (0.0, -0.1, 1.0000001, 2.0, nan, inf, -inf):
        for flags in (0, 1):
            assert call(blend=bad, flags=flags) == E and "blend is not finite and in (0, 1]" in text(), bad
    assert text().startswith("crender_taa_resolve: ")
    # the order
    assert call(col=None, vel=None, H=0, y0=9, flags=2, out=hist, blend=nan) == E and "is NULL" in text()
    assert call(vel=None, H=0, y0=9, flags=2, out=hist, blend=nan) == E and "d_z without d_velocity" in text()
    assert call(H=0, y0=9, flags=2, out=hist, blend=nan) == E and "H or W is below 1" in text()
    assert call(y0=9, flags=2, out=hist, blend=nan) == E and "rows outside the frame" in text()
    assert call(flags=2, out=hist, blend=nan) == E and "unknown flag bits" in text()
    assert call(out=hist, blend=nan) == E and "d_out is d_color or d_history" in text()


# ---- section 1: the jitter -------------------------------------------------------------------------------------

PROJ = np.float32([[2.4, 0, 0, 0], [0, 2.4, 0, 0], [0, 0, 1.0002, 1.0], [0, 0, -0.2, 0]])      # a matrix of the shape


def test_jitter_offsets_view_shear_and_sheared():
    o = taa_ref.jitter_offsets(6)
    assert o.dtype == np.float64 and o.shape == (6, 2)
    assert o[:, 0].tolist() == [0.0, -0.25, 0.25, -0.375, 0.125, -0.125]
    assert np.allclose(o[:, 1], np.array([1, 2, 1 / 3, 4 / 3, 7 / 3, 2 / 3]) / 3 - 0.5, atol=1e-15)
    big = taa_ref.jitter_offsets(64)
    assert (big >= -0.5).all() and (big < 0.5).all() and len({tuple(p) for p in big}) == 64
    assert_bit_equal(big[:6].astype(np.float32), o.astype(np.float32), "a longer cycle starts alike")
    assert taa_ref.jitter_offsets(0).shape == (0, 2)
    kx, ky = taa_ref.view_shear(PROJ, 100, 60, 0.25, -0.375)
    assert type(kx) is np.float32 and type(ky) is np.float32
    assert kx == np.float32(0.25 / (30.0 * float(np.float32(2.4)))) and ky == np.float32(-0.375 / (50.0 * float(np.float32(2.4))))
    assert taa_ref.view_shear(PROJ.reshape(16), 100, 60, 0.25, -0.375) == (kx, ky)
    v = np.random.default_rng(3).uniform(-2, 2, (50, 3, 3)).astype(np.float32)
    s = taa_ref.sheared(v, kx, ky)
    assert s is not v and s.dtype == np.float32 and s.shape == v.shape
    assert_bit_equal(s[..., 2], v[..., 2], "z")
    assert_bit_equal(s[..., 0], v[..., 0] + v[..., 2] * kx, "x")
    assert_bit_equal(s[..., 1], v[..., 1] + v[..., 2] * ky, "y")
    t = taa_ref.sheared(torch.from_numpy(v), kx, ky)
    assert isinstance(t, torch.Tensor)
    assert_bit_equal(t.numpy(), s, "the torch form")
    # the image moves by (jx, jy) pixels: the projection of the sheared corners
    v[..., 2] = np.abs(v[..., 2]) + 0.5
    import tex_ref
    moved = tex_ref.project(taa_ref.sheared(v, kx, ky), PROJ, 60, 100) - tex_ref.project(v, PROJ, 60, 100)
    assert np.abs(moved[..., 0] - 0.25).max() < 1e-4 and np.abs(moved[..., 1] + 0.375).max() < 1e-4
    for bad in (v.astype(np.float64), v[0], [[1.0]]):
        with pytest.raises(ValueError, match="vertices must be"):
            taa_ref.sheared(bad, kx, ky)


# ---- section 2: the model on hand-made planes ------------------------------------------------------------------

def _planes(H, W, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 255, (H, W, 3)).astype(np.float32), rng.uniform(0, 255, (H, W, 3)).astype(np.float32)


def test_blend_one_and_off_frame_positions_copy_bits():
    color, hist = _planes(9, 11)
    color[4, 5].view(np.uint32)[:] = [0x7FC00123, 0xFFC00001, 0x80000000]       # NaN payloads and -0
    assert_bit_equal(taa_ref.resolve(color, hist, blend=1.0), color, "blend = 1")
    vel = np.zeros((9, 11, 2), np.float32)
    vel[4, 5] = (6, 0)             # px = -1: off the left side
    vel[4, 6] = (-5, 0)            # px = 11: off the right
    vel[2, 3] = (0, 3)             # py = -1: above
    vel[7, 3] = (0, -2)            # py = 9: below
    vel[4, 2] = (2, 0)             # px = 0 exactly: counts
    vel[4, 8] = (-2, 0)            # px = W - 1 exactly: counts
    vel[4, 3] = (3.5, 0)           # px = -0.5: does not
    vel[4, 9] = (-1.5, 0)          # px = 10.5: does not
    c = {}
    got = taa_ref.resolve(color, hist, vel, blend=0.25, counts=c)
    for y, x in ((4, 5), (4, 6), (2, 3), (7, 3), (4, 3), (4, 9)):
        assert_bit_equal(got[y, x], color[y, x], f"off the frame at {(y, x)}")
    assert c["kept"] == 6 and c["four"] == 0
    plain = taa_ref.resolve(color, hist, blend=0.25, flags=1)
    vgot = taa_ref.resolve(color, hist, vel, blend=0.25, flags=1)
    keep = np.float32(0.75)
    assert_bit_equal(vgot[4, 2], color[4, 2] + (hist[4, 0] - color[4, 2]) * keep, "px = 0 reads column 0")
    assert_bit_equal(vgot[4, 8], color[4, 8] + (hist[4, 10] - color[4, 8]) * keep, "px = W - 1 reads the last column")
    assert_bit_equal(plain, color + (hist - color) * keep, "a static view without the clamp")
    # a strip: its own rows are the frame's edge, and the rows outside keep what `out` held
    sentinel = np.full((9, 11, 3), -7, np.float32)
    vel[:] = 0
    vel[3, 4], vel[6, 4], vel[5, 4] = (0, 1), (0, -1), (0, 2)          # py = 2: outside; py = 7: outside; py = 3: the first row
    strip = taa_ref.resolve(color, hist, vel, blend=0.5, y0=3, y1=7, out=sentinel, flags=1)
    assert (strip[:3] == -7).all() and (strip[7:] == -7).all()
    assert_bit_equal(strip[3, 4], color[3, 4], "above the strip")
    assert_bit_equal(strip[6, 4], color[6, 4], "below the strip")
    assert_bit_equal(strip[5, 4], color[5, 4] + (hist[3, 4] - color[5, 4]) * np.float32(0.5), "the strip's first row counts")


def test_the_history_sample():
    color, hist = _planes(8, 8, 2)
    vel = np.zeros((8, 8, 2), np.float32)
    vel[3, 3] = (0.5, 0.25)        # px = 2.5, py = 2.75
    vel[5, 5] = (1, -1)            # whole pixels: one texel, and the NaNs beside it are not seen
    vel[6, 2] = (0.5, 0)           # fy == 0: the row below is not seen
    vel[1, 7] = (0, -0.5)          # the last column: ix1 is clamped to it
    hist[6, 5], hist[6, 3], hist[7, 4] = NAN, NAN, NAN           # around (6, 4), which (5, 5) reads
    hist[7, 1], hist[7, 2] = NAN, NAN                            # below what (6, 2) reads
    got = taa_ref.resolve(color, hist, vel, blend=0.5, flags=1)
    half = np.float32(0.5)
    top = hist[2, 2] + (hist[2, 3] - hist[2, 2]) * half
    bot = hist[3, 2] + (hist[3, 3] - hist[3, 2]) * half
    h = top + (bot - top) * np.float32(0.75)
    assert_bit_equal(got[3, 3], color[3, 3] + (h - color[3, 3]) * half, "four taps")
    assert_bit_equal(got[5, 5], color[5, 5] + (hist[6, 4] - color[5, 5]) * half, "fx == 0 and fy == 0")
    h = hist[6, 1] + (hist[6, 2] - hist[6, 1]) * half
    assert_bit_equal(got[6, 2], color[6, 2] + (h - color[6, 2]) * half, "fy == 0")
    h = hist[1, 7] + (hist[2, 7] - hist[1, 7]) * half
    assert_bit_equal(got[1, 7], color[1, 7] + (h - color[1, 7]) * half, "the last column")
    # the NaNs reach only the five still pixels that hold them
    assert sorted(zip(*np.nonzero(np.isnan(got).any(2)))) == [(6, 3), (6, 5), (7, 1), (7, 2), (7, 4)]
    # non-finite velocities count as none
    vel[:] = 0
    vel[2, 2], vel[2, 3], vel[2, 4] = (NAN, 1), (INF, 0), (1, -INF)
    assert_bit_equal(taa_ref.resolve(color, _planes(8, 8, 2)[1], vel, blend=0.5), taa_ref.resolve(color, _planes(8, 8, 2)[1], blend=0.5),
                     "odd velocities")


def test_the_dilation_ties_go_to_the_pixel_then_to_the_first_neighbour():
    z = np.full((5, 5), 3, np.float32)
    sy, sx = taa_ref.dilated_source(z)
    assert (sy == np.arange(5)[:, None]).all() and (sx == np.arange(5)[None, :]).all()         # all equal: p itself
    z[1, 3] = z[3, 1] = z[2, 3] = 1                                       # three equal nearer ones around (2, 2)
    sy, sx = taa_ref.dilated_source(z)
    assert (sy[2, 2], sx[2, 2]) == (1, 3)                                 # the first in row-major order
    assert (sy[1, 3], sx[1, 3]) == (1, 3) and (sy[2, 3], sx[2, 3]) == (2, 3)      # p wins its own tie
    z[1, 1] = NAN
    z[2, 1] = -INF
    sy, sx = taa_ref.dilated_source(z)
    assert (sy[2, 2], sx[2, 2]) == (2, 1) and (sy[1, 1], sx[1, 1]) == (1, 1)      # a NaN neither replaces nor is replaced
    # the strip does not see across its edge, the frame neither
    z[:] = 3
    z[0, 2] = z[4, 2] = 1
    sy, sx = taa_ref.dilated_source(z, 1, 4)
    assert (sy == np.arange(1, 4)[:, None]).all()
    # and the velocity is read there
    color, hist = _planes(5, 5, 4)
    vel = np.zeros((5, 5, 2), np.float32)
    vel[1, 3] = (1, 0)
    z[:] = 3
    z[1, 3] = 1
    got = taa_ref.resolve(color, hist, vel, z, blend=0.5, flags=1)
    assert_bit_equal(got[2, 2], color[2, 2] + (hist[2, 1] - color[2, 2]) * np.float32(0.5), "the neighbour's velocity")
    plain = taa_ref.resolve(color, hist, vel, None, blend=0.5, flags=1)
    assert_bit_equal(plain[2, 2], color[2, 2] + (hist[2, 2] - color[2, 2]) * np.float32(0.5), "its own without d_z")


def test_the_box_keeps_the_result_between_lo_and_hi():
    rng = np.random.default_rng(5)
    for H, W, y0, y1 in ((33, 47, 0, 33), (20, 9, 3, 17), (1, 12, 0, 1), (12, 1, 0, 12)):
        color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
        hist = rng.uniform(-500, 800, (H, W, 3)).astype(np.float32)       # nothing to do with the frame
        vel = rng.uniform(-3, 3, (H, W, 2)).astype(np.float32)
        z = rng.uniform(0, 1, (H, W)).astype(np.float32)
        lo, hi = taa_ref.box(color, y0, y1)
        assert (lo <= color[y0:y1]).all() and (color[y0:y1] <= hi).all()
        if H > 2 and W > 2 and (y0, y1) == (0, H):
            assert lo[1, 1, 0] == color[0:3, 0:3, 0].min() and hi[1, 1, 2] == color[0:3, 0:3, 2].max()
            assert lo[0, 0, 1] == color[0:2, 0:2, 1].min()                # the corner's four
        for blend in (0.05, 0.5, 0.999):
            got = taa_ref.resolve(color, hist, vel, z, blend=blend, y0=y0, y1=y1)[y0:y1]
            # c + (hc - c) * keep with lo <= c, hc <= hi and 0 < keep < 1: within the box up to the three roundings
            slack = np.float32(2.0 ** -22) * np.maximum(np.abs(lo), np.abs(hi))
            assert (got >= lo - slack).all() and (got <= hi + slack).all(), (H, W, blend)
            if blend == 0.05 and H * W > 20:               # and without the box it leaves it
                loose = taa_ref.resolve(color, hist, vel, z, blend=blend, y0=y0, y1=y1, flags=1)[y0:y1]
                assert ((loose < lo - 1) | (loose > hi + 1)).any()


# ---- the model on the oracle's frames --------------------------------------------------------------------------

def _lit_frame(oracle, arrays, H, W, jx, jy):
    """(the oracle's filler with the frame of `arrays` moved by (jx, jy) pixels and lit, the sheared vertices, the shear)."""
    tri, col, nrm = arrays
    f = oracle.OracleFiller(H, W, fov=45.0)
    k = taa_ref.view_shear(f.proj_mat, H, W, jx, jy)
    sv = taa_ref.sheared(tri, *k)
    f.render_arrays(sv, col, nrm)
    oracle.guro(f.color_buffer, f.normals_buffer, LIGHT)
    return f, sv, k


def _truth(oracle, arrays, H, W, g):
    """The float64 mean of the g x g grid of jittered frames."""
    acc = np.zeros((H, W, 3), np.float64)
    for i in range(g):
        for j in range(g):
            acc += _lit_frame(oracle, arrays, H, W, (i + 0.5) / g - 0.5, (j + 0.5) / g - 0.5)[0].color_buffer
    return acc / (g * g)


J = 16       # the length of the offset cycle of the two prototypes


@pytest.mark.parametrize("side,found", [(64, 0.275), (128, 0.324)])
def test_a_still_trex_converges_towards_the_supersampled_image(oracle, side, found):
    """16 jittered frames of the still T-Rex, resolved with blend max(0.1, 1 / (n + 1)) and the clamp: the mean absolute
    error against the 8 x 8 truth is at most half the plain frame's (found: 0.275 of it at 64^2, 0.324 at 128^2)."""
    arrays = trex_arrays()
    truth = _truth(oracle, arrays, side, side, 8)
    plain = float(np.abs(_lit_frame(oracle, arrays, side, side, 0, 0)[0].color_buffer - truth).mean())
    offsets = taa_ref.jitter_offsets(J)
    hist = None
    for n in range(16):
        frame = _lit_frame(oracle, arrays, side, side, *offsets[n % J])[0].color_buffer
        hist = frame.copy() if n == 0 else taa_ref.resolve(frame, hist, blend=max(0.1, 1.0 / (n + 1)))
    after = float(np.abs(hist - truth).mean())
    print(f"T-Rex {side}^2: plain {plain:.3f}, after 16 frames {after:.3f}: {after / plain:.3f} of it")
    assert after <= 0.5 * plain
    assert abs(after / plain - found) < 0.002             # what this file's README figures say


@pytest.fixture(scope="module")
def turning(oracle):
    """The 128^2 prototype under motion: T-Rex turning 2 degrees about y per frame, 17 poses -> {variant: (the error against
    the 6 x 6 truth at the last pose, the last step's (colour, history, velocity, z))}."""
    H = W = 128
    tri, col, nrm = trex_arrays()
    poses = [motion_ref.rotated(tri, (0, 2 * i, 0)) for i in range(17)]
    truth = _truth(oracle, (poses[-1], col, nrm), H, W, 6)
    offsets = taa_ref.jitter_offsets(J)
    frames = []
    for n, pose in enumerate(poses):
        f, sv, k = _lit_frame(oracle, (pose, col, nrm), H, W, *offsets[n % J])
        vel = None if n == 0 else motion_ref.motion_vectors(f.winner, sv, f.proj_mat, taa_ref.sheared(poses[n - 1], *k))
        frames.append((f.color_buffer, vel, f.z_buffer))
    got = {}
    for name, reproject, dilate, flags in (("dilated", True, True, 0), ("reprojected", True, False, 0), ("static", False, False, 0),
                                           ("reprojected, no clamp", True, False, 1), ("static, no clamp", False, False, 1)):
        hist = frames[0][0].copy()
        for n in range(1, 17):
            color, vel, z = frames[n]
            last = (color, hist, vel if reproject else None, z if dilate else None)
            hist = taa_ref.resolve(*last, blend=max(0.1, 1.0 / (n + 1)), flags=flags)
        got[name] = (float(np.abs(hist - truth).mean()), last)
    got["plain"] = (float(np.abs(_lit_frame(oracle, (poses[-1], col, nrm), H, W, 0, 0)[0].color_buffer - truth).mean()), None)
    return got


def test_the_orderings_under_motion(turning):
    e = {k: v[0] for k, v in turning.items()}
    print("T-Rex 128^2 turning 2 degrees a frame, error against the 6 x 6 truth:", {k: round(v, 3) for k, v in e.items()})
    assert e["dilated"] < e["reprojected"] < e["static"]
    assert e["reprojected"] < e["reprojected, no clamp"] and e["static"] < e["static, no clamp"]


F64_MEASURED = 1.136e-4     # largest |float32 - float64| of a resolve step over the frames of `turning` (see the test)


def test_float32_against_float64(turning):
    """The same statements in float64 from the same float32 inputs, on the last step of every variant of the turning
    T-Rex: two lerps and a blend on colours up to 255, a handful of roundings of 2^-24 each; where px falls within a
    rounding of a whole pixel the two evaluations may take another texel pair, whose weights then differ by that rounding
    as well.  The bound is ten times the largest measured difference: the margin is for frames not measured.  A check of
    the model's statements, not a bound on the kernel, which is held to bit equality with the float32 model."""
    worst = 0.0
    for name, (_, last) in turning.items():
        if last is None:
            continue
        for flags in (0, 1):
            o32 = taa_ref.resolve(*last, blend=0.1, flags=flags)
            o64 = taa_ref.resolve(*last, blend=0.1, flags=flags, dtype=np.float64)
            assert o32.dtype == np.float32 and o64.dtype == np.float64 and not np.isnan(o64).any()
            d = float(np.abs(o32.astype(np.float64) - o64).max())
            print(f"{name}, flags {flags}: largest |out - out64| = {d:.3e}")
            worst = max(worst, d)
    print(f"largest over the frames: {worst:.3e} (bound {10 * F64_MEASURED:.3e})")
    assert 0 < worst <= 10 * F64_MEASURED


# ---- the Python layer, on CPU tensors --------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses  # noqa: E402


class FakeFiller(fake_filler_base()):
    """The protocol of the two mixins on CPU tensors; the launch is the host model."""

    def _launch_pass(self, entry, args):
        if entry == VECTORS:
            winner, tri, T, pos_of, P, prev, exposure, out, h, w, y0, y1, flags = args
            self.events.append((entry, T, exposure, flags))
            got = motion_ref.motion_vectors(winner.numpy(), tri.numpy(), P, prev.numpy(), exposure, y0, y1, out=out.numpy())
        else:
            assert entry == RESOLVE
            color, hist, vel, z, blend, out, h, w, y0, y1, flags = args
            self.events.append((entry, vel is not None, z is not None, blend, flags))
            assert color is self.color_buffer and out is not color and out is not hist
            assert z is None or z is self.z_buffer
            assert type(blend) is float and (h, w, y0, y1) == (self.h, self.w, self.y0, self.y1)
            got = taa_ref.resolve(color.numpy(), hist.numpy(), None if vel is None else vel.numpy(),
                                  None if z is None else z.numpy(), blend, y0, y1, flags, out=out.numpy())
        out.copy_(torch.from_numpy(got))


class _Frame(Frame):
    pass


SOUPS = {71: (3000, 256, 256, (3.0, 50.0))}
soups = soups_fixture(_Frame, SOUPS)


def test_temporal_resolve_returns_a_new_tensor_and_leaves_the_views_as_they_were(soups):
    s = soups[71]
    T = len(s.tri)
    cam = s.cam
    prev = motion_ref.rotated(s.tri, (0, 0, 2))
    hist = np.random.default_rng(6).uniform(0, 255, (s.H, s.W, 3)).astype(np.float32)
    f = FakeFiller(s)
    # no history: the frame, copied
    out = f.temporal_resolve(None)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out is not f.color_buffer
    assert_bit_equal(out.numpy(), cam.color_buffer, "no history")
    assert f.events == ["push", "settle"]
    # a static view: no velocity plane is made or read
    f.events.clear()
    out = f.temporal_resolve(hist, blend=0.25)
    assert f.events == ["push", "settle", (RESOLVE, False, False, 0.25, 0)]
    assert_bit_equal(out.numpy(), taa_ref.resolve(cam.color_buffer, hist, blend=0.25), "a static view")
    f.events.clear()
    f.temporal_resolve(torch.from_numpy(hist), dilate=False, clamp=False)
    assert f.events == ["push", "settle", (RESOLVE, False, False, float(np.float32(0.1)), 1)]
    # the previous pose: the motion vectors at exposure 1, then the resolve with the z plane
    vel = motion_ref.motion_vectors(cam.winner, s.tri, cam.proj_mat, prev)
    f.events.clear()
    out = f.temporal_resolve(hist, prev, blend=0.5)
    assert f.events == ["push", "settle", (VECTORS, T, 1.0, 0), "push", "settle", (RESOLVE, True, True, 0.5, 0)]
    want = taa_ref.resolve(cam.color_buffer, hist, vel, cam.z_buffer, blend=0.5)
    assert (want != cam.color_buffer).any()
    assert_bit_equal(out.numpy(), want, "previous_vertices")
    assert_bit_equal(f.temporal_resolve(hist, torch.from_numpy(prev), blend=0.5).numpy(), want, "previous_vertices, a tensor")
    assert_bit_equal(f.temporal_resolve(hist, velocity=vel, blend=0.5).numpy(), want, "velocity=, numpy")
    f.events.clear()
    got = f.temporal_resolve(hist, velocity=torch.from_numpy(vel), blend=0.5, dilate=False, clamp=False)
    assert f.events == ["push", "settle", (RESOLVE, True, False, 0.5, 1)]
    assert_bit_equal(got.numpy(), taa_ref.resolve(cam.color_buffer, hist, vel, blend=0.5, flags=1), "neither dilated nor clamped")
    assert not f._host_fresh and not f._host_exposed
    assert_bit_equal(f.color_buffer.numpy(), cam.color_buffer, "the colour plane is only read")
    assert_bit_equal(f.z_buffer.numpy(), cam.z_buffer, "the z plane is only read")
    sig = inspect.signature(DeferredPasses.temporal_resolve)
    assert [(p.name, p.default, p.kind == p.KEYWORD_ONLY) for p in sig.parameters.values()][1:] == \
        [("history", inspect.Parameter.empty, False), ("previous_vertices", None, False), ("velocity", None, True),
         ("blend", 0.1, True), ("dilate", True, True), ("clamp", True, True)]
    # an edit made in a view is carried up first
    view = f.get_color_buffer()
    view[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    f.events.clear()
    again = f.temporal_resolve(hist, velocity=vel, blend=0.5)
    assert f.events[0] == "push" and f._host_fresh
    edited = cam.color_buffer.copy()
    edited[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    assert_bit_equal(again.numpy(), taa_ref.resolve(edited, hist, vel, cam.z_buffer, blend=0.5), "over the edited colours")
    # a row strip fills its rows and leaves the others zero
    g = FakeFiller(s, row_strip=(37, 75))
    strip = g.temporal_resolve(hist, prev, blend=0.5).numpy()
    assert not strip[:37].any() and not strip[75:].any()
    vs = motion_ref.motion_vectors(cam.winner, s.tri, cam.proj_mat, prev, y0=37, y1=75)
    assert_bit_equal(strip[37:75], taa_ref.resolve(cam.color_buffer, hist, vs, cam.z_buffer, blend=0.5, y0=37, y1=75)[37:75], "the strip")
    none = g.temporal_resolve(None).numpy()
    assert not none[:37].any() and not none[75:].any()
    assert_bit_equal(none[37:75], cam.color_buffer[37:75], "the strip, no history")


def test_temporal_resolve_refuses_what_motion_blur_refuses_and_names_bad_arguments(soups):
    s = soups[71]
    prev = motion_ref.rotated(s.tri, (0, 0, 2))
    hist = np.zeros((s.H, s.W, 3), np.float32)
    name = "temporal_resolve"
    f = FakeFiller(s)
    f._pipeline = object()
    with pytest.raises(ValueError, match=name + r" is not available on a swap chain \(pipeline=True\)"):
        f.temporal_resolve(hist)
    with pytest.raises(ValueError, match=name + " needs the winner plane"):
        FakeFiller(s, track_winner=False).temporal_resolve(hist)
    f = FakeFiller(s)
    f._inputs = None
    with pytest.raises(ValueError, match=name + ": no frame has been rendered"):
        f.temporal_resolve(hist)
    f = FakeFiller(s)
    f._last_flags = 0
    with pytest.raises(ValueError, match=name + ": the last frame did not start from cleared buffers"):
        f.temporal_resolve(hist)
    f = FakeFiller(s)
    T = len(s.tri)
    v = np.zeros((s.H, s.W, 2), np.float32)
    with pytest.raises(ValueError, match="at most one of previous_vertices and velocity"):
        f.temporal_resolve(hist, prev, velocity=v)
    for bad in (hist[1:], hist[..., :2], hist.astype(np.float64), v):
        with pytest.raises(ValueError, match=rf"history must be None or float32 \[{s.H}, {s.W}, 3\], the frame's, got"):
            f.temporal_resolve(bad)
    for bad in (v[1:], v[..., :1], v.astype(np.float64), hist):
        with pytest.raises(ValueError, match=rf"velocity must be float32 \[{s.H}, {s.W}, 2\], the frame's, got"):
            f.temporal_resolve(hist, velocity=bad)
    with pytest.raises(ValueError, match=f"{name}: previous_vertices holds {T - 1} triangles, the last frame drew {T}"):
        f.temporal_resolve(hist, prev[1:])
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'float' but got 'double'"):
        f.temporal_resolve(hist, prev.astype(np.float64))
    for bad in (0, 0.0, -0.5, 1.5, float("nan"), float("inf"), 1e-50, True, "1", None):
        with pytest.raises(ValueError, match="blend must be a number above 0 and at most 1, got " + re.escape(repr(bad))):
            f.temporal_resolve(hist, blend=bad)
    for key in ("dilate", "clamp"):
        for bad in (0, 1, None, "yes"):
            with pytest.raises(ValueError, match=f"{key} must be a bool, got " + re.escape(repr(bad))):
                f.temporal_resolve(hist, **{key: bad})
    assert f.events == []                                                 # nothing was pushed, settled or launched
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    assert AdvancedPixelBufferFiller.temporal_resolve is DeferredPasses.temporal_resolve


# ---- the Renderer ----------------------------------------------------------------------------------------------

H8 = W8 = 8


def _resolved(f, history, previous_vertices=None, **kw):
    """What the recording filler's pass returns: a fresh tensor per call, numbered."""
    f.count = getattr(f, "count", 0) + 1
    return torch.full((H8, W8, 3), float(f.count))


_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass phong_pass shade_guro bloom get_color_tensor get_color_buffer temporal_resolve "
    "texture_pass bind_texture",
    returns=dict(bloom="bloomed", temporal_resolve=_resolved), quiet="_push_host_edits synchronize get_normals_buffer", _P=PROJ)


def _shear(n, cycle):
    return taa_ref.view_shear(PROJ, H8, W8, *taa_ref.jitter_offsets(cycle)[n % cycle])


def test_renderer_construction():
    from cython3dmodelrenderer_amd.renderer import Renderer
    names = list(inspect.signature(Renderer.__init__).parameters)
    assert "temporal_aa" in names and inspect.signature(Renderer.__init__).parameters["temporal_aa"].default is None
    assert Renderer(SimpleNamespace(), None).temporal_aa is None

    class Plain:
        pass

    class History:
        def temporal_resolve(self, history, **kw):
            pass

        depth_of_field = edge_aa = resolve = transparency_pass = motion_blur = bloom = temporal_resolve
    with pytest.raises(ValueError, match=r"Renderer\(temporal_aa=\.\.\.\) needs a filler with a temporal resolve pass "
                                         r"\(AdvancedPixelBufferFiller\): Plain has no temporal_resolve\(\)"):
        Renderer(Plain(), None, temporal_aa={})
    clash = (r"Renderer\(temporal_aa=\.\.\.\) together with antialias=\.\.\., depth_of_field=\.\.\., motion_blur=\.\.\., "
             r"supersample=\.\.\. or transparency=\.\.\.: each of them reads the filler's own colour plane and would not see "
             r"the resolved one; use one of them")
    for other in (dict(antialias={}), dict(depth_of_field=dict(focus=1.0)), dict(motion_blur={}), dict(supersample=2),
                  dict(transparency=dict(alpha=0.5))):
        with pytest.raises(ValueError, match=clash):
            Renderer(History(), None, temporal_aa={}, **other)
    with pytest.raises(ValueError, match=r"Renderer\(temporal_aa=\.\.\.\) takes the keys 'blend', 'jitter', 'dilate' and 'clamp': "
                                         r"\['frames'\] unknown"):
        Renderer(History(), None, temporal_aa=dict(frames=2))
    for bad in (-1, 65, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match=r"jitter must be an int from 0 to 64, got " + re.escape(repr(bad))):
            Renderer(History(), None, temporal_aa=dict(jitter=bad))
    for bad in (0, -0.1, 1.5, float("nan"), True, None):
        with pytest.raises(ValueError, match=r"blend must be a number above 0 and at most 1, got " + re.escape(repr(bad))):
            Renderer(History(), None, temporal_aa=dict(blend=bad))
    opts = dict(blend=0.2, jitter=16, dilate=False, clamp=False)
    r = Renderer(History(), None, temporal_aa=opts)
    assert r.temporal_aa == opts and r.temporal_aa is not opts and r._cleared
    assert Renderer(History(), None, temporal_aa={}).temporal_aa == {}
    assert Renderer(History(), None, temporal_aa={}, bloom={}, wireframe=None).bloom == {}       # bloom combines


def test_renderer_jitters_the_frames_and_resolves_them_against_the_call_before():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    pose0 = np.arange(18, dtype=np.float32).reshape(2, 3, 3) + 1
    colours, normals = np.zeros((2, 3, 3), np.float32), np.ones((2, 3, 3), np.float32)
    model = SimpleNamespace(_vertices_by_triangles=pose0.copy(), _colors_by_triangles=colours, _normals_by_triangles=normals)
    guro = GuroIllumination(LIGHT)
    f = _Recorder(H8, W8)
    r = Renderer(f, guro, on_device="fused", temporal_aa=dict(jitter=3, blend=0.3, dilate=False))
    images, poses = [], []
    for n in range(5):
        poses.append(model._vertices_by_triangles.copy())
        images.append(r.render(model))
        model._vertices_by_triangles += 1                  # the model moves IN PLACE
    assert [c[0] for c in f.calls][:4] == ["set_fused_illumination", "render_model", "get_color_tensor", "temporal_resolve"]
    draws = [c for c in f.calls if c[0] == "render_model"]
    passes = [c for c in f.calls if c[0] == "temporal_resolve"]
    assert len(draws) == len(passes) == 5 and all(c[2].get("clear") is True for c in draws)
    for n in range(5):
        # the offsets in order and their wrap at 3: the stand-in carries the sheared vertices, the other arrays as they are
        drawn = draws[n][1][0]
        assert drawn is not model and drawn._colors_by_triangles is colours and drawn._normals_by_triangles is normals
        assert_bit_equal(drawn._vertices_by_triangles, taa_ref.sheared(poses[n], *_shear(n, 3)), f"frame {n}: the drawn vertices")
        assert images[n] is not None and torch.equal(images[n], torch.full((H8, W8, 3), float(n + 1)))
    assert _shear(3, 3) == _shear(0, 3) != _shear(1, 3)
    assert passes[0][1] == (None,) and passes[0][2] == {}                  # frame 0: the jittered frame, copied
    for n in range(1, 5):
        (history,), kw = passes[n][1], passes[n][2]
        assert history is images[n - 1]                                   # the tensor it returned is the next history
        assert set(kw) == {"previous_vertices", "blend", "dilate"} and kw["dilate"] is False
        assert kw["blend"] == max(0.3, 1.0 / (n + 1))                     # 1/2, 1/3, then the floor
        # the previous UNJITTERED pose, sheared by THIS frame's offset
        assert_bit_equal(kw["previous_vertices"].numpy(), taa_ref.sheared(poses[n - 1], *_shear(n, 3)), f"frame {n}: the previous pose")
    assert [p[2]["blend"] for p in passes[1:]] == [0.5, 1.0 / 3, 0.3, 0.3]
    # reset_motion: frame 0 again, offset 0 again
    r.reset_motion()
    f.calls.clear()
    pose = model._vertices_by_triangles.copy()
    r.render(model)
    assert f.calls[-1][:2] == ("temporal_resolve", (None,))
    assert_bit_equal(f.calls[1][1][0]._vertices_by_triangles, taa_ref.sheared(pose, *_shear(0, 3)), "after the reset")
    r.render(model)
    assert f.calls[-1][2]["blend"] == 0.5
    # another triangle count: frame 0 of the new count
    model._vertices_by_triangles = np.ones((5, 3, 3), np.float32)
    model._colors_by_triangles = model._normals_by_triangles = np.ones((5, 3, 3), np.float32)
    f.calls.clear()
    r.render(model)
    assert f.calls[-1][:2] == ("temporal_resolve", (None,))
    assert_bit_equal(f.calls[1][1][0]._vertices_by_triangles, taa_ref.sheared(model._vertices_by_triangles, *_shear(0, 3)), "a new count")
    r.render(model)
    assert f.calls[-1][2]["blend"] == 0.5 and tuple(f.calls[-1][2]["previous_vertices"].shape) == (5, 3, 3)
    # a tensor model stays a tensor; jitter=0 draws the model itself and leaves the previous pose as it was
    model._vertices_by_triangles = torch.ones((5, 3, 3))
    f = _Recorder(H8, W8)
    r = Renderer(f, guro, on_device=True, temporal_aa=dict(jitter=0))
    r.render(model)
    assert f.calls[1][1][0] is model
    model._vertices_by_triangles += 1
    got = r.render(model)
    assert isinstance(got, torch.Tensor) and f.calls[-1][0] == "temporal_resolve"
    assert (f.calls[-1][2]["previous_vertices"] == 1).all() and f.calls[-1][2]["blend"] == 0.5
    assert [c[0] for c in f.calls[-5:]] == ["set_fused_illumination", "render_model", "shade_guro", "get_color_tensor", "temporal_resolve"]
    # None and False return a fresh numpy copy
    for on_device in (None, False):
        f = _Recorder(H8, W8)
        r = Renderer(f, guro, on_device=on_device, temporal_aa={})
        for n in range(2):
            got = r.render(model)
            assert isinstance(got, np.ndarray) and (got == n + 1).all()
        assert f.calls[-1][0] == "temporal_resolve" and isinstance(f.calls[-1][1][0], torch.Tensor)
    # a PhongIllumination, and bloom after the pass, over its tensor; the history stays the pass's own
    f = _Recorder(H8, W8)
    r = Renderer(f, PhongIllumination(position=(0.0, 0.0, 1.0)), on_device=True, temporal_aa={}, bloom={})
    assert r.render(model) == "bloomed"
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "phong_pass", "get_color_tensor", "temporal_resolve", "bloom"]
    first = f.calls[-1][2]["source"]
    assert torch.equal(first, torch.full((H8, W8, 3), 1.0))
    assert r.render(model) == "bloomed"
    assert f.calls[-2][1][0] is first and torch.equal(f.calls[-1][2]["source"], torch.full((H8, W8, 3), 2.0))
    # the helpers keep receiving the caller's model
    class Textured:
        _vertices_by_triangles, _colors_by_triangles, _normals_by_triangles = pose0.copy(), colours, normals
        get_texture_coords_by_triangles, get_texture = staticmethod(lambda: "uv"), staticmethod(lambda: "texture")
    textured = Textured()
    f = _Recorder(H8, W8)
    Renderer(f, guro, on_device="fused", temporal_aa={}, texture_pass={}).render(textured)
    assert ("bind_texture", ("uv", "texture"), {}) in f.calls and f.calls[[c[0] for c in f.calls].index("render_model")][1][0] is not textured
    # without the option nothing changes
    f = _Recorder(H8, W8)
    assert Renderer(f, guro, on_device="fused").render(model) == "colour"
    assert "temporal_resolve" not in [c[0] for c in f.calls] and f.calls[1][1][0] is model and f.calls[1][2] == dict(clear=True)
