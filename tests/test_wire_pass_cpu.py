"""The hidden-line overlay without a GPU: the header against the binding and the build lists, the entry point's
argument checks, the host model the GPU tests compare with (tests/overlay_ref.py) pinned on the oracle's frames by
counts, by identities and against a float64 evaluation, ``wireframe.feature_edges``, and ``Renderer(wireframe=...)``."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import overlay_ref
from pass_scenes import Frame, capi, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from util import LIBRARY_SOURCES, UNIT_KEYS, assert_bit_equal, other_symbols, unit_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAY_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_float),
                    C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                    C.c_uint, C.c_void_p]


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_overlay_symbol_is_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_wire.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert "crender_wire_overlay" in declared and declared == set(capi.UNIT_SIGNATURES["wire"])
    assert not declared & other_symbols(capi, "wire")
    res, args = capi.UNIT_SIGNATURES["wire"]["crender_wire_overlay"]
    assert res == C.c_int and args == OVERLAY_ARGTYPES
    assert capi.load().crender_wire_overlay.argtypes == OVERLAY_ARGTYPES
    decl = re.search(r"CRENDER_API int crender_wire_overlay\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(args) == 18
    kinds = ["float" if re.match(r"\s*float \w+$", a) else "other" for a in decl.split(",")]
    assert [i for i, k in enumerate(kinds) if k == "float"] == [i for i, a in enumerate(args) if a is C.c_float] == [8, 9, 10]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert "crender_wire_overlay" in set(re.findall(r" T (crender_\w+)", out))
    limits = dict(re.findall(r"#define (CRENDER_WIRE_\w+) (\d+)", header))
    assert int(limits["CRENDER_WIRE_MAX_WIDTH"]) == capi.WIRE_MAX_WIDTH == overlay_ref.MAX_WIDTH == 64
    assert capi.ABI_VERSION == 6


def test_the_build_lists_are_unchanged():
    from cython3dmodelrenderer_amd import _build
    assert _build.source_sha16() == "35a9bf480abfca1e"
    assert _build.library_sources() == LIBRARY_SOURCES
    assert list(_build.UNITS) == UNIT_KEYS
    assert _build.UNITS["wire"][0] == ["wireframe.hip"]
    # the overlay's kernel takes the passes' frame from the shared header, which a unit of its own watches
    inputs = _build.build_inputs()
    assert unit_inputs(_build, "wire") | unit_inputs(_build, "pass") <= set(inputs) and len(inputs) == len(set(inputs))
    unit = open(os.path.join(_build.SRC_DIR, "wireframe.hip")).read()
    assert '#include "winner_pass.h"' in unit
    # (the gather and the projection of a winner's corners are the header's winner_triangle)
    for name in ("winner_triangle(", "make_proj(", "wave_any(", "winner_pixel(", "tile_origin(", "pass_grid("):
        assert name in unit and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name
    for name in ("project_vertex(", "gather_corners("):
        assert name not in unit, name


def test_overlay_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    nan, inf = float("nan"), float("inf")
    white = (C.c_float * 3)(255.0, 255.0, 255.0)
    grey = (C.c_float * 3)(40.0, 40.0, 40.0)

    def overlay(win=fake, tri=fake, T=4, pos_of=None, P=P, edges=None, line=white, fill=None, width=1.0, feather=1.0,
                opacity=1.0, col=fake, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_wire_overlay(win, tri, T, pos_of, P, edges, line, fill, width, feather, opacity, col,
                                      H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(P=None), dict(line=None), dict(col=None)):
        assert overlay(**kw) == E and "is NULL" in text(), kw
    assert overlay(tri=None) == E and "NULL with T > 0" in text()
    assert overlay(T=-1) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2)):
        assert overlay(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert overlay(**kw) == E and "rows outside the frame" in text(), kw
    for name in ("width", "feather"):
        for bad in (nan, inf, -inf, 0.0, -1.0, 64.5, 1e30):
            assert overlay(**{name: bad}) == E and f"{name} is not in (0, 64]" in text(), (name, bad)
    for bad in (nan, inf, -inf, -0.001, 1.001):
        assert overlay(opacity=bad) == E and "opacity is not in [0, 1]" in text(), bad
    for bad in (nan, inf, -inf):
        for i in range(3):
            c = [255.0] * 3
            c[i] = bad
            assert overlay(line=(C.c_float * 3)(*c)) == E and "not finite" in text(), (bad, i)
            assert overlay(fill=(C.c_float * 3)(*c)) == E and "not finite" in text(), (bad, i)
    for flags in (1, 2, 0x80000000):
        assert overlay(flags=flags) == E and "unknown flag bits" in text(), flags
    assert text().startswith("crender_wire_overlay")
    # the ends of the ranges are inside; without triangles there is nothing to launch
    assert overlay(T=0, tri=None) == capi.OK
    assert overlay(T=0, width=64.0, feather=64.0, opacity=0.0, fill=grey, edges=fake) == capi.OK
    assert overlay(T=0, width=1e-30, feather=1e-30) == capi.OK
    assert overlay(T=0, width=65.0) == E


# ---- the model on the oracle's frames --------------------------------------------------------------------------

class _Frame(Frame):
    def run(self, **kw):
        return overlay_ref.wire_pass(self.cam.color_buffer, self.cam.winner, self.tri, self.cam.proj_mat, **kw)

    def distances(self, **kw):
        return overlay_ref.distances(self.cam.winner, self.tri, self.cam.proj_mat, **kw)[3]


SOUPS = {61: (300, 40, 37, (3.0, 25.0)), 51: (4000, 200, 173, (1.0, 40.0)), 71: (3000, 256, 256, (3.0, 50.0))}


soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)


# (covered, (a >= 1, 0 < a < 1, off) at width 1 / feather 1, the same at width 3 / feather 0.5) from the host model
COUNTS = {61: (1476, (0, 708, 768), (826, 172, 478)),
          51: (34592, (0, 11227, 23365), (13402, 3774, 17416)),
          71: (65439, (0, 16961, 48478), (20386, 5966, 39087))}


@pytest.mark.parametrize("seed", [61, 51, 71])
def test_the_counts_on_the_soups(soups, seed):
    f = soups[seed]
    covered, thin, wide = COUNTS[seed]
    for (width, feather), want in (((1.0, 1.0), thin), ((3.0, 0.5), wide)):
        c = {}
        out = f.run(width=width, feather=feather, counts=c)
        assert (c["covered"], (c["full"], c["partial"], c["off"])) == (covered, want), (width, feather, c)
        assert c["nan"] == 0 and not np.isnan(out).any()
        assert_bit_equal(out[~f.covered], f.cam.color_buffer[~f.covered], "the background is not written")
    # what the scenes are chosen for: at width 3 / feather 0.5 all three classes are well represented
    assert min(wide) >= 0.05 * covered


def test_the_counts_on_trex(trex):
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    c = {}
    trex.run(counts=c)
    assert c == dict(covered=15801, full=0, partial=14275, off=1526, nan=0)      # every edge: a grey smear
    mask = feature_edges(trex.tri, 30.0)
    trex.run(edges=mask, counts=c)
    assert c == dict(covered=15801, full=0, partial=3145, off=12656, nan=0)
    trex.run(edges=mask, width=3.0, feather=0.5, counts=c)
    assert c == dict(covered=15801, full=3520, partial=621, off=11660, nan=0)


@pytest.mark.parametrize("seed,measured", [(51, 3.72e-6), (71, 4.44e-6)])
def test_the_distances_against_float64(soups, seed, measured):
    """The same statements from the same float32 projected corners in float64, no pixel excluded.  Measured with this
    model: the largest |m - m64| is 3.711e-6 pixels on seed 51 and 4.434e-6 on seed 71 (corners up to a few hundred
    pixels from the pixel, one float32 rounding of each product).  The bound is four times the measured value: the
    margin is for other frames of the same scale.  It is a check of the model's statements, not a bound on the kernel,
    which is held to bit equality with the float32 model."""
    f = soups[seed]
    m32, m64 = f.distances(), f.distances(dtype=np.float64)
    assert m32.dtype == np.float32 and m64.dtype == np.float64 and np.isfinite(m64).all()
    diff = float(np.abs(m32.astype(np.float64) - m64).max())
    print(f"seed {seed}: largest |m - m64| = {diff:.3e} pixels (bound {4 * measured:.3e})")
    assert 0 < diff <= 4 * measured
    # and the colours: a is m / feather, a colour 255 * a
    a = f.run(width=3.0, feather=0.5)
    b = f.run(width=3.0, feather=0.5, dtype=np.float64)
    assert b.dtype == np.float64
    # |da| <= |dm| / feather plus float32's roundings of a, k and the blend (values up to 255: 4 roundings of 2^-24 * 256)
    assert np.abs(a.astype(np.float64) - b).max() <= 255 * (4 * measured) / 0.5 + 4 * 2.0 ** -16


def test_identities(soups):
    f = soups[71]
    base = f.cam.color_buffer
    T = len(f.tri)
    none = np.zeros(T, np.uint8)
    fill = (10.0, 20.0, 30.0)
    # a mask of 0 everywhere: nothing without a fill, the fill everywhere covered with it
    assert_bit_equal(f.run(edges=none, width=3.0), base, "no edge drawn")
    c = {}
    out = f.run(edges=none, fill=fill, counts=c)
    assert c["off"] == c["covered"] == int(f.covered.sum())
    assert (out[f.covered] == np.float32(fill)).all()
    assert_bit_equal(out[~f.covered], base[~f.covered], "the fill leaves the background alone")
    # bits 3 to 7 are ignored
    assert_bit_equal(f.run(edges=np.full(T, 0xF8, np.uint8)), base, "bits 3 to 7")
    assert_bit_equal(f.run(edges=np.full(T, 0xFF, np.uint8)), f.run(), "all bits against no mask")
    # widening never removes a line pixel
    on = None
    for width in (0.5, 1.0, 2.0, 3.0, 8.0):
        ys, xs, _, m, _ = overlay_ref.distances(f.cam.winner, f.tri, f.cam.proj_mat)
        hi = np.float32(width) * np.float32(0.5) + np.float32(0.5) * np.float32(0.5)
        now = (hi - m) / np.float32(0.5) > 0
        assert on is None or (now[on]).all()
        assert on is None or now.sum() > on.sum()
        on = now
    # opacity 0 without a fill leaves the values (c * 1 + line * 0)
    assert np.array_equal(f.run(width=3.0, opacity=0.0), base)
    # a pixel with all of the opacity is the line's colour; the fill shows through half of it at opacity 0.5
    rng = np.random.default_rng(5)
    mask = rng.integers(0, 8, T).astype(np.uint8)
    c = {}
    out = f.run(width=3.0, feather=0.5, line=(1.0, 2.0, 3.0), edges=mask, counts=c)
    assert c["full"] > 1000 and int((out == np.float32([1.0, 2.0, 3.0])).all(2).sum()) >= c["full"]
    half = f.run(width=3.0, feather=0.5, line=(100.0, 200.0, 50.0), fill=(0.0, 0.0, 100.0), opacity=0.5, edges=mask)
    assert int((half == np.float32([50.0, 100.0, 75.0])).all(2).sum()) == c["full"]
    # rows: the pass over two strips is the pass over the frame
    top = f.run(width=2.0, y0=0, y1=100)
    both = overlay_ref.wire_pass(top, f.cam.winner, f.tri, f.cam.proj_mat, width=2.0, y0=100, y1=256)
    assert_bit_equal(both, f.run(width=2.0), "two strips")
    assert_bit_equal(top[100:], base[100:], "rows below the strip")


# ---- feature edges ---------------------------------------------------------------------------------------------

def _half_edges(mask):
    return int(np.unpackbits(mask[:, None] & 7, axis=1).sum())


def test_feature_edges():
    from cython3dmodelrenderer_amd import scenes
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    cube = scenes.load_fixture("cube_inputs.npz")[0]
    mask = feature_edges(cube, 30.0)
    assert mask.dtype == np.uint8 and mask.tolist() == [3, 6, 3, 6, 3, 6, 3, 6, 3, 6, 3, 6]      # no face's diagonal
    assert feature_edges(cube, 0.0).tolist() == mask.tolist() == feature_edges(cube, 89.0).tolist()
    assert feature_edges(cube, 91.0).tolist() == [0] * 12
    trex = scenes.load_fixture("trex_inputs.npz")[0]
    mask = feature_edges(trex)
    # (the vectorised form gives the counts of the loop it replaced)
    assert len(mask) == 13814 and _half_edges(mask) == 10122 and int((mask == 0).sum()) == 5819
    assert _half_edges(feature_edges(trex, 0.0)) > _half_edges(mask) > _half_edges(feature_edges(trex, 60.0)) > 0
    # the order of the triangles does not matter, nor which corner comes first
    perm = np.random.default_rng(3).permutation(len(trex))
    assert np.array_equal(feature_edges(trex[perm]), mask[perm])
    rolled = feature_edges(trex[:, [1, 2, 0]])
    assert np.array_equal(rolled, ((mask >> 1) | (mask << 2)) & 7)
    # borders, faces without area, edges of three faces
    one = np.float32([[[0, 0, 1], [1, 0, 1], [0, 1, 1]]])
    assert feature_edges(one).tolist() == [7]
    quad = np.float32([[[0, 0, 1], [1, 0, 1], [1, 1, 1]], [[0, 0, 1], [1, 1, 1], [0, 1, 1]]])
    assert feature_edges(quad).tolist() == [3, 6]                        # the diagonal is hidden, the border drawn
    assert feature_edges(quad[:, ::-1]).tolist() == [3, 5]               # the other winding: the diagonal is edge 2, edge 1
    sliver = quad.copy()
    sliver[1, 2] = sliver[1, 1]                                          # the second face has no area
    assert feature_edges(sliver)[0] == 7
    fin = np.concatenate([quad, np.float32([[[0, 0, 1], [1, 1, 1], [0.5, 0.5, 0]]])])
    assert (feature_edges(fin)[:2] == 7).all()                           # the diagonal now has two partners
    assert feature_edges(np.zeros((0, 3, 3), np.float32)).shape == (0,)
    with pytest.raises(ValueError, match=r"\[T, 3, 3\]"):
        feature_edges(np.zeros((4, 3), np.float32))


# ---- the Renderer ----------------------------------------------------------------------------------------------

def test_renderer_option():
    from cython3dmodelrenderer_amd.renderer import Renderer
    names = list(inspect.signature(Renderer.__init__).parameters)
    assert names.index("wireframe") == names.index("supersample") - 1 and names[-1] == "supersample"
    assert Renderer(SimpleNamespace(), None).wireframe is None

    class Plain:
        pass

    class WithPass:
        def wire_pass(self):
            pass
    with pytest.raises(ValueError, match="Plain has no wire_pass"):
        Renderer(Plain(), None, wireframe={})
    opts = dict(width=2.0, feature_angle=30)
    r = Renderer(WithPass(), None, wireframe=opts)
    assert r.wireframe == opts and r.wireframe is not opts


def test_wire_pass_refuses_bad_arguments_before_it_looks_at_the_device():
    """The checks of the Python layer on a stand-in that has no device at all."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses

    class Stub(DeferredPasses):
        _pipeline = None
        winner_buffer = object()
        _inputs = (np.zeros((5, 3, 3), np.float32),)
        _last_flags = 1
    for kw, word in ((dict(width=0), "width"), (dict(width=64.5), "width"), (dict(width=float("nan")), "width"),
                     (dict(feather=0.0), "feather"), (dict(feather=-1), "feather"), (dict(feather=float("inf")), "feather"),
                     (dict(opacity=-0.1), "opacity"), (dict(opacity=1.5), "opacity"), (dict(opacity=float("nan")), "opacity"),
                     (dict(width="1"), "width")):
        with pytest.raises(ValueError, match=word):
            Stub().wire_pass(**kw)
    with pytest.raises(ValueError, match=r"T = 5.*\(4,\)"):
        Stub().wire_pass(edges=np.zeros(4, np.uint8))
    with pytest.raises(ValueError, match=r"T = 5.*int32.*\(5,\)"):
        Stub().wire_pass(edges=np.zeros(5, np.int32))
    chain = Stub()
    chain._pipeline = object()
    with pytest.raises(ValueError, match="swap chain"):
        chain.wire_pass()
