"""Transparency without a GPU: the header against the binding and the library, the unit's place in the build tables, the
two entry points' argument checks and their order; the host model the GPU tests compare with (tests/peel_ref.py) pinned
on the oracle's frames — layer 0 is the oracle's frame, every triangle's fragments are what the oracle draws of it alone,
the counts per layer — and on an analytic scene, its blend against its own float64 evaluation;
``AdvancedPixelBufferFiller.peel_layers`` and ``transparency_pass``'s protocol on CPU tensors and
``Renderer(transparency=...)``."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import peel_ref
from pass_scenes import LIGHT, Frame, Soup, capi, fake_filler_base, recording_filler, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from util import assert_bit_equal, other_symbols, own_unit_source, random_soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEXT, BLEND = "crender_peel_next", "crender_peel_blend"
_vp, _i32, _f32p = C.c_void_p, C.c_int, C.POINTER(C.c_float)
NEXT_ARGTYPES = [_vp, _vp, _vp, C.c_int64, _vp, _f32p, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.c_uint, _vp]
BLEND_ARGTYPES = [_vp, _vp, C.c_int64, _vp, _f32p, _vp, _vp, _vp, _f32p, _vp, _f32p, _vp, _vp, _i32, _i32, _i32, _i32,
                  C.c_uint, _vp]
NEXT_PARAMS = ["const int32_t *d_winner", "const float *d_z", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of",
               "const float *P16", "const float *d_nrm", "void *d_keys", "int32_t *d_winner_out", "float *d_z_out", "int H",
               "int W", "int y0", "int y1", "unsigned flags", "void *stream"]
BLEND_PARAMS = ["const int32_t *d_winner", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of", "const float *P16",
                "const float *d_col", "const float *d_nrm", "const float *d_alpha", "const float *light3",
                "const float *d_front", "const float *background3", "float *d_trans", "float *d_out", "int H", "int W",
                "int y0", "int y1", "unsigned flags", "void *stream"]


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_peel_symbols_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_peel.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["peel"]) == {NEXT, BLEND}
    assert not declared & other_symbols(capi, "peel")
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    exported = set(re.findall(r" T (crender_\w+)", out))
    for entry, argtypes, params in ((NEXT, NEXT_ARGTYPES, NEXT_PARAMS), (BLEND, BLEND_ARGTYPES, BLEND_PARAMS)):
        assert entry in exported
        res, args = capi.UNIT_SIGNATURES["peel"][entry]
        assert res == C.c_int and args == argtypes == getattr(capi.load(), entry).argtypes
        decl = re.search(r"CRENDER_API int " + entry + r"\((.*?)\);", header, re.S).group(1)
        assert [" ".join(a.split()) for a in decl.split(",")] == params and len(params) == len(args)
    assert "/* ---- Transparency" in header
    top = int(re.search(r"#define CRENDER_PEEL_MAX_LAYERS (\d+)", header).group(1))
    assert top == capi.PEEL_MAX_LAYERS == peel_ref.MAX_LAYERS == 16
    assert int(re.search(r"#define CRENDER_PEEL_FIRST (\d+)u", header).group(1)) == capi.PEEL_FIRST == 1
    assert int(re.search(r"#define CRENDER_PEEL_LAST (\d+)u", header).group(1)) == capi.PEEL_LAST == 2
    assert capi.ABI_VERSION == 6 and capi.load().crender_abi_version() == 6


def test_peel_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit = new = own_unit_source(_build, "peel", "peel.hip", "crender_peel.h")
    head = "// ---- transparency (crender_peel_next, crender_peel_blend) ----"
    assert unit.count(head) == 1
    assert unit.index(head) < unit.index("void k_peel_seed") < unit.index("void k_peel_cover") \
        < unit.index("void k_peel_resolve") < unit.index("void k_peel_blend") < unit.index("int crender_peel_next(") \
        < unit.index("int crender_peel_blend(")
    # a unit of its own: its namespace and its entry points, the passes' frame from the shared header as it is
    assert new.count("namespace {") == 1 and new.count('extern "C" {') == 1
    for name in ("winner_triangle(", "winner_pixel(", "barycentric(", "make_proj(", "wave_any(", "pass_grid(", "frame_checks(",
                 "rows_check(", "arg_error("):
        assert name in new and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name
    assert "project_vertex(" not in unit and "gather_corners(" not in unit
    assert "CR_DEV" not in new and "asm" not in new and "__shared__" not in new and "__syncthreads" not in new
    # raster_math.h as it is
    for name in ("backface(", "pixel_box(", "fragment(", "fragment_key(", "zord(", "make_key(", "KEY_LOW_PRIOR", "interp(",
                 "shade_fragment("):
        assert name in new, name
    # the cover pass: both tests with plain loads, then the one atomic; the grid cap the GPU test's second trip relies on
    cover = new[new.index("void k_peel_cover"):new.index("void k_peel_resolve")]
    assert cover.count("atomicMin(") == 1 and cover.index("k < *slot") < cover.index("K < k") < cover.index("atomicMin(")
    assert "constexpr int kPeelMaxGrid = 8192;" in new and "grid_for((size_t)T * 64, kPeelMaxGrid)" in new
    assert new.index("frame_checks(E") < new.index("rows_check(E") < new.index("unknown flag bits")


def _P(capi):
    return capi.f32_16(np.float32([[2.4, 0, 0, 0], [0, 2.4, 0, 0], [0, 0, 1.0002, 1.0], [0, 0, -0.2, 0]]))


def test_peel_next_argument_errors_without_a_gpu(capi):
    L, E = capi.load(), capi.EINVAL
    P = _P(capi)
    fake, other, third = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)     # never dereferenced

    def peel(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=P, nrm=fake, keys=fake, wout=other, zout=third, H=8, W=8, y0=0,
             y1=8, flags=0):
        return L.crender_peel_next(win, z, tri, T, pos_of, P, nrm, keys, wout, zout, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(z=None), dict(P=None), dict(keys=None), dict(wout=None), dict(zout=None)):
        assert peel(**kw) == E and "d_winner, d_z, P16, d_keys, d_winner_out or d_z_out is NULL" in text(), kw
    for bad in (-1, -2 ** 40):
        assert peel(T=bad) == E and "T is negative" in text()
    for kw in (dict(tri=None), dict(nrm=None)):
        assert peel(**kw) == E and "d_tri or d_nrm is NULL with T > 0" in text(), kw
    for kw in (dict(H=0), dict(W=-2), dict(H=-2 ** 31)):
        assert peel(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert peel(**kw) == E and "rows outside the frame" in text(), kw
    for flags in (1, 2, 0x80000000):
        assert peel(flags=flags) == E and "unknown flag bits" in text(), flags
    assert peel(T=2 ** 31) == E and "T is above 2^31 - 1" in text()
    for kw in (dict(wout=fake), dict(zout=fake)):
        assert peel(**kw) == E and "an output plane is its input" in text(), kw
    assert text().startswith("crender_peel_next: ")
    # the order: the pointers, T, the triangle arrays, the frame, the rows, the flags, T's top, the aliasing
    assert peel(win=None, T=-1, H=0, y0=9, flags=1, wout=fake) == E and "is NULL" in text() and "d_winner," in text()
    assert peel(T=-1, tri=None, H=0, y0=9, flags=1, wout=fake) == E and "T is negative" in text()
    assert peel(tri=None, H=0, y0=9, flags=1, wout=fake) == E and "d_tri or d_nrm is NULL" in text()
    assert peel(H=0, y0=9, flags=1, wout=fake) == E and "H or W is below 1" in text()
    assert peel(y0=9, flags=1, wout=fake) == E and "rows outside the frame" in text()
    assert peel(flags=1, T=2 ** 31, wout=fake) == E and "unknown flag bits" in text()
    assert peel(T=2 ** 31, wout=fake) == E and "T is above" in text()
    assert peel(wout=fake) == E and "an output plane is its input" in text()


def test_peel_blend_argument_errors_without_a_gpu(capi):
    L, E = capi.load(), capi.EINVAL
    P = _P(capi)
    fake, other, third = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)     # never dereferenced
    nan, inf = float("nan"), float("inf")
    f3 = lambda *v: (C.c_float * 3)(*v)                                       # noqa: E731

    def blend(win=fake, tri=fake, T=4, pos_of=None, P=P, col=fake, nrm=fake, alpha=fake, light=None, front=None,
              bg=f3(0, 0, 0), trans=other, out=third, H=8, W=8, y0=0, y1=8, flags=1):
        return L.crender_peel_blend(win, tri, T, pos_of, P, col, nrm, alpha, light, front, bg, trans, out, H, W, y0, y1, flags,
                                    None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(P=None), dict(bg=None), dict(trans=None), dict(out=None)):
        assert blend(**kw) == E and "d_winner, P16, background3, d_trans or d_out is NULL" in text(), kw
    assert blend(T=-1) == E and "T is negative" in text()
    for kw in (dict(tri=None), dict(col=None), dict(nrm=None), dict(alpha=None)):
        assert blend(**kw) == E and "d_tri, d_col, d_nrm or d_alpha is NULL with T > 0" in text(), kw
    for kw in (dict(H=0), dict(W=-2)):
        assert blend(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3)):
        assert blend(**kw) == E and "rows outside the frame" in text(), kw
    for flags in (4, 5, 0x80000000):
        assert blend(flags=flags) == E and "unknown flag bits" in text(), flags
    for flags in (0, 2):
        assert blend(front=fake, flags=flags) == E and "d_front is given without CRENDER_PEEL_FIRST" in text(), flags
    assert blend(front=third) == E and "d_out is d_front" in text()
    for bad in (nan, inf, -inf):
        assert blend(bg=f3(0, bad, 0)) == E and "background3 is not finite" in text(), bad
        assert blend(light=f3(0, 0, bad)) == E and "light3 is not finite" in text(), bad
    assert text().startswith("crender_peel_blend: ")
    # the order
    bad = dict(bg=f3(nan, 0, 0), light=f3(nan, 0, 0))
    assert blend(win=None, T=-1, H=0, y0=9, flags=4, **bad) == E and "is NULL" in text() and "d_winner," in text()
    assert blend(T=-1, tri=None, H=0, y0=9, flags=4, **bad) == E and "T is negative" in text()
    assert blend(tri=None, H=0, y0=9, flags=4, **bad) == E and "with T > 0" in text()
    assert blend(H=0, y0=9, flags=4, **bad) == E and "H or W is below 1" in text()
    assert blend(y0=9, flags=4, **bad) == E and "rows outside the frame" in text()
    assert blend(flags=4, front=fake, **bad) == E and "unknown flag bits" in text()
    assert blend(flags=2, front=third, **bad) == E and "without CRENDER_PEEL_FIRST" in text()
    assert blend(front=third, **bad) == E and "d_out is d_front" in text()
    assert blend(**bad) == E and "background3 is not finite" in text()
    assert blend(light=f3(nan, 0, 0)) == E and "light3 is not finite" in text()


# ---- the model on the oracle's frames --------------------------------------------------------------------------

class _Frame(Frame):
    """The oracle's frame and, computed once, the model's fragments of it."""
    _frags = None

    @property
    def frags(self):
        if self._frags is None:
            self._frags = peel_ref.fragments(self.tri, self.nrm, self.cam.proj_mat, self.H, self.W)
        return self._frags


SOUPS = {51: (4000, 200, 173, (1.0, 40.0)), 8: (3000, 256, 256, (3.0, 50.0))}

soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)


@pytest.fixture(scope="module")
def soup71(oracle):
    m = Soup()
    return _Frame(oracle, (m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles), 256, 256)


def _per_layer(frags, n):
    return [int((frags.rank == k).sum()) for k in range(n)]


def test_layer_0_is_the_oracles_frame_and_the_counts(trex, soup71, soups):
    for name, f in (("trex", trex), ("soup 71", soup71), ("soup 51", soups[51]), ("soup 8", soups[8])):
        w, z = peel_ref.layers(f.frags, 2)
        assert_bit_equal(w[0], f.cam.winner, f"{name}: layer 0's winners")
        assert_bit_equal(z[0], f.cam.z_buffer, f"{name}: layer 0's z")
        # and the colours a frame stores for layer 0 are the model's shade of it
        assert_bit_equal(peel_ref.shade(w[0], f.tri, f.col, f.nrm, f.cam.proj_mat), f.cam.color_buffer, f"{name}: colours")
        print(f"{name}: {len(f.frags)} fragments, depth {f.frags.depth}, per layer {_per_layer(f.frags, min(f.frags.depth, 8))}")
        assert (w[1] >= 0).sum() > 0 and not ((w[1] >= 0) & (w[0] < 0)).any()
    assert (len(trex.frags), trex.frags.depth) == (19808, 5)
    assert _per_layer(trex.frags, 5) == [15801, 3197, 683, 110, 17]
    assert (len(soup71.frags), soup71.frags.depth) == (400606, 19) and soup71.frags.depth >= 8
    assert _per_layer(soup71.frags, 8) == [65439, 64668, 61786, 55946, 46989, 36264, 26171, 17676]


def test_keys_strictly_increase_and_peeling_is_the_sort(trex, soup71):
    for f in (trex, soup71):
        fr = f.frags
        same = fr.pix[1:] == fr.pix[:-1]
        assert (fr.key[1:][same] > fr.key[:-1][same]).all() and (fr.key < peel_ref.CLEAR_KEY).all()
        # no adjacent layers of a pixel share a z in these scenes: the tie case has a scene of its own on the GPU
        assert not (fr.z[1:][same] == fr.z[:-1][same]).any()
        n = min(fr.depth + 1, 7)
        w, z = peel_ref.layers(fr, n)
        for k in range(1, n):
            wk, zk = peel_ref.peel_next(fr, w[k - 1], z[k - 1])
            assert_bit_equal(wk, w[k], f"layer {k}: winners")
            assert_bit_equal(zk, z[k], f"layer {k}: z")
        if n > fr.depth:
            assert (w[-1] == -1).all() and (z[-1] == np.float32(1e6)).all()
        # an exhausted pixel stays exhausted
        wk, zk = peel_ref.peel_next(fr, *peel_ref.empty_layer(f.H, f.W))
        assert (wk == -1).all() and (zk == np.float32(1e6)).all()


def test_every_triangle_alone_is_its_fragments(oracle):
    """An independent enumeration: the oracle renders each triangle of a small soup ALONE; what it covers, with its z, are
    the model's fragments of that triangle, and the per-pixel sort of those by key gives the model's layers."""
    H = W = 64
    tri, col, nrm = random_soup(np.random.default_rng(5), 40, 64, size_px=(4.0, 40.0))
    ref = oracle.OracleFiller(H, W, fov=45.0)
    fr = peel_ref.fragments(tri, nrm, ref.proj_mat, H, W)
    assert fr.depth >= 4 and len(fr) > 2000
    per_pixel = [[] for _ in range(H * W)]
    total = 0
    for i in range(len(tri)):
        one = oracle.OracleFiller(H, W, fov=45.0)
        one.render_arrays(tri[i:i + 1], col[i:i + 1], nrm[i:i + 1])
        pix = np.nonzero(one.winner.ravel() == 0)[0]
        mine = fr.idx == i
        order = np.argsort(fr.pix[mine])
        assert np.array_equal(fr.pix[mine][order], pix), i
        assert_bit_equal(fr.z[mine][order], one.z_buffer.ravel()[pix], f"triangle {i}: z")
        total += len(pix)
        for p, z in zip(pix, one.z_buffer.ravel()[pix]):
            per_pixel[p].append((int(peel_ref.fragment_key(z, i)), i, z))
    assert total == len(fr)
    n = fr.depth
    w, z = peel_ref.layers(fr, n)
    for p, found in enumerate(per_pixel):
        found.sort()
        for k in range(n):
            want = found[k] if k < len(found) else (0, -1, np.float32(1e6))
            assert w[k].ravel()[p] == want[1] and z[k].ravel()[p].view(np.uint32) == np.float32(want[2]).view(np.uint32), (p, k)


# ---- the blend ---------------------------------------------------------------------------------------------------

def test_blend_identities(trex):
    f = trex
    P, T = f.cam.proj_mat, len(f.tri)
    ground = (10.0, 20.0, 30.0)
    front = f.cam.color_buffer.copy()
    front[f.covered] = np.where(np.random.default_rng(2).uniform(size=(int(f.covered.sum()), 3)) < 0.2, np.float32(-0.0),
                                front[f.covered])
    # alpha = 1: the front colours bit for bit, -0 included, the background elsewhere; whatever lies behind
    behind = f.col.copy()
    behind[:] = np.nan
    want = front.copy()
    want[~f.covered] = ground
    for n in (1, 4):
        got = peel_ref.transparency(f.frags, f.tri, behind, f.nrm, P, 1.0, n, background=ground, front=front)
        assert_bit_equal(got, want, f"alpha = 1, {n} layers")
    assert (np.signbit(want) & (want == 0)).sum() > 1000
    # alpha = 0: the background everywhere
    got = peel_ref.transparency(f.frags, f.tri, f.col, f.nrm, P, 0.0, 5, background=ground)
    assert_bit_equal(got, np.broadcast_to(np.float32(ground), got.shape), "alpha = 0")
    # an opaque layer in the middle: triangles behind it are never blended, their NaN colours do not spread
    w, _ = peel_ref.layers(f.frags, 5)
    opaque = np.unique(w[1][w[1] >= 0])
    alpha = np.full(T, 0.5, np.float32)
    alpha[opaque] = 1.0
    col = f.col.copy()
    only_behind = np.setdiff1d(np.unique(w[2:][w[2:] >= 0]), np.unique(w[:2][w[:2] >= 0]))
    assert len(only_behind) > 10
    col[only_behind] = np.nan
    two_deep = (w[2] >= 0) & np.isin(w[1], opaque) & np.isin(w[2], only_behind)
    assert two_deep.sum() > 20
    got = peel_ref.transparency(f.frags, f.tri, col, f.nrm, P, alpha, 5, background=ground)
    assert not np.isnan(got[two_deep]).any()
    assert_bit_equal(got[two_deep], peel_ref.transparency(f.frags, f.tri, col, f.nrm, P, alpha, 2, background=ground)[two_deep],
                     "nothing behind the opaque layer is added")
    # alpha is clamped, a NaN is 0
    assert_bit_equal(peel_ref.clamp_alpha(np.float32([-1, -0.0, 0.25, 1, 7, np.nan, np.inf])), np.float32([0, 0, 0.25, 1, 1, 0, 1]),
                     "the clamp")


F64_MEASURED = 4.478e-5              # measured with this model: 1.398e-5 on T-Rex, 4.434e-5 on seed 71, 4.478e-5 on seed 51


def test_float32_blend_against_float64(trex, soup71, soups):
    """The blend's statements in float64 from the same float32 inputs (alpha, every layer's float32 colours, the
    background), 8 layers, random alpha, colours 0 .. 255, a background, with the light.  A pixel is a sum of at most 9
    terms, each a product of at most 8 factors below 1 and a colour: roundings of 2^-24 relative each on values up to
    255.  The bound is ten times the largest measured difference: the margin is for frames not measured.  A check of
    the model's statements, not a bound on the kernel, which is held to bit equality with the float32 model."""
    worst = 0.0
    light = np.float32([0.3, -0.2, -1.0]) / np.linalg.norm(np.float32([0.3, -0.2, -1.0]))
    for name, f in (("trex", trex), ("soup71", soup71), ("soup51", soups[51])):
        alpha = np.random.default_rng(11).uniform(0, 1, len(f.tri)).astype(np.float32)
        kw = dict(n=8, light=light, background=(10.0, 20.0, 30.0))
        o32 = peel_ref.transparency(f.frags, f.tri, f.col, f.nrm, f.cam.proj_mat, alpha, **kw)
        o64 = peel_ref.transparency(f.frags, f.tri, f.col, f.nrm, f.cam.proj_mat, alpha, dtype=np.float64, **kw)
        assert o32.dtype == np.float32 and o64.dtype == np.float64 and not np.isnan(o64).any()
        diff = float(np.abs(o32.astype(np.float64) - o64).max())
        print(f"{name}: largest |out - out64| = {diff:.3e}")
        worst = max(worst, diff)
    print(f"largest |out - out64| over the three frames = {worst:.3e} (bound {10 * F64_MEASURED:.3e})")
    assert 0 < worst <= 10 * F64_MEASURED


def test_three_stacked_quads_in_closed_form(oracle):
    """Three quads that fill a 32 x 32 frame at depths 1, 2 and 3 with alpha 1/2, 1/4 and 1 and one colour each: every
    pixel is c1 / 2 + c2 / 8 + 3 c3 / 8.  The quads' diagonals run half a pixel off the pixel centres, so that every pixel
    has three fragments.  The interpolation of one colour c over a triangle is c (b1 + b2 + b3) with three rounded
    barycentrics and two rounded sums: within 255 * 8 * 2^-24 of c, and the three terms' errors add: 1e-3 holds with a
    margin of ten."""
    H = W = 32
    P = oracle.OracleFiller(H, W, fov=45.0).proj_mat
    assert P[0, 1] == P[1, 0] == P[3, 0] == P[3, 1] == 0

    def corner(x, y, depth):
        return [(x / (W / 2.0) - 1.0) * depth / float(P[0, 0]), (y / (H / 2.0) - 1.0) * depth / float(P[1, 1]), depth]
    tri, col = [], []
    colours = [(200.0, 100.0, 50.0), (40.0, 80.0, 160.0), (16.0, 255.0, 8.0)]
    for depth, c in zip((1.0, 2.0, 3.0), colours):
        A, B, Cc, D = (corner(-8, -8.5, depth), corner(W + 8, -8.5, depth), corner(W + 8, W + 7.5, depth),
                       corner(-8, W + 7.5, depth))
        tri += [[A, B, Cc], [A, Cc, D]]
        col += [[c] * 3] * 2
    tri, col = np.float32(tri), np.float32(col)
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1.0
    fr = peel_ref.fragments(tri, nrm, P, H, W)
    assert len(fr) == 3 * H * W and fr.depth == 3 and _per_layer(fr, 3) == [H * W] * 3
    w, z = peel_ref.layers(fr, 4)
    assert (w[0] < 2).all() and ((w[1] == 2) | (w[1] == 3)).all() and (w[2] >= 4).all() and (w[3] == -1).all()
    alpha = np.float32([0.5, 0.5, 0.25, 0.25, 1.0, 1.0])
    want = np.float32(colours[0]) / 2 + np.float32(colours[1]) / 8 + 3 * np.float32(colours[2]) / 8
    for n in (3, 4):
        got = peel_ref.transparency(fr, tri, col, nrm, P, alpha, n, background=(255.0, 255.0, 255.0))
        assert np.abs(got - want).max() <= 1e-3
    # two layers: the third's share shows the background
    got = peel_ref.transparency(fr, tri, col, nrm, P, alpha, 2, background=(255.0, 0.0, 255.0))
    want2 = np.float32(colours[0]) / 2 + np.float32(colours[1]) / 8 + 3 * np.float32([255.0, 0.0, 255.0]) / 8
    assert np.abs(got - want2).max() <= 1e-3


# ---- the Python layer, on CPU tensors --------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses  # noqa: E402


class FakeFiller(fake_filler_base()):
    """The protocol of the two mixins on CPU tensors; the launches are the host model."""

    inputs = ("tri", "col", "nrm")

    def _launch_pass(self, entry, args):
        f = self.frame
        if entry == NEXT:
            winner, z, tri, T, pos_of, P, nrm, keys, w_out, z_out, h, w, y0, y1, flags = args
            self.events.append((entry, T, flags))
            assert keys.dtype == torch.int64 and keys.numel() * 8 == 8 * h * w and w_out is not winner and z_out is not z
            assert tri is self._inputs[0] and nrm is self._inputs[2] and pos_of is None and flags == 0
            got = peel_ref.peel_next(f.frags, winner.numpy(), z.numpy(), None, y0, y1, out=(w_out.numpy(), z_out.numpy()))
            w_out.copy_(torch.from_numpy(got[0]))
            z_out.copy_(torch.from_numpy(got[1]))
            return
        assert entry == BLEND
        winner, tri, T, pos_of, P, col, nrm, alpha, light, front, ground, trans, out, h, w, y0, y1, flags = args
        self.events.append((entry, T, flags, front is not None, None if light is None else tuple(light), tuple(ground)))
        assert col is self._inputs[1] and nrm is self._inputs[2] and alpha.dtype == torch.float32 and tuple(alpha.shape) == (T,)
        assert front is None or front is self.color_buffer
        colour = front.numpy() if front is not None else \
            peel_ref.shade(winner.numpy(), f.tri, f.col, f.nrm, P, None if light is None else list(light), y0, y1)
        peel_ref.blend(out.numpy(), trans.numpy(), winner.numpy(), T, alpha.numpy(), colour, bool(flags & 1), bool(flags & 2),
                       list(ground), None, y0, y1)


def test_peel_layers_on_a_fake_filler(soup71):
    s = soup71
    T = len(s.tri)
    f = FakeFiller(s)
    w, z = f.peel_layers(4)
    assert w.dtype == torch.int32 and z.dtype == torch.float32 and tuple(w.shape) == tuple(z.shape) == (4, 256, 256)
    assert f.events == ["push", "settle"] + [(NEXT, T, 0)] * 3              # edits, the settle, the launches
    want = peel_ref.layers(s.frags, 4)
    assert_bit_equal(w.numpy(), want[0], "winners")
    assert_bit_equal(z.numpy(), want[1], "z")
    assert not f._host_fresh and not f._host_exposed                       # the planes are only read
    assert_bit_equal(f.winner_buffer.numpy(), s.cam.winner, "the winner plane is only read")
    assert_bit_equal(f.z_buffer.numpy(), s.cam.z_buffer, "the z plane is only read")
    scratch = f._peel_scratch
    f.events.clear()
    one = f.peel_layers(1)
    assert f.events == ["push", "settle"] and f._peel_scratch is scratch    # layer 0 is a copy; the scratch is kept
    assert_bit_equal(one[0][0].numpy(), s.cam.winner, "layer 0")
    assert one[0].data_ptr() != f.winner_buffer.data_ptr()
    # a row strip fills its rows and leaves the others zero
    g = FakeFiller(s, row_strip=(37, 75))
    w, z = g.peel_layers(3)
    assert not w[:, :37].any() and not w[:, 75:].any() and not z[:, :37].any() and not z[:, 75:].any()
    assert_bit_equal(w[:, 37:75].numpy(), want[0][:3, 37:75], "the strip's rows")
    for bad in (0, 17, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="n must be an int from 1 to 16, got " + re.escape(repr(bad))):
            f.peel_layers(bad)


def test_transparency_pass_on_a_fake_filler(soup71):
    s = soup71
    T = len(s.tri)
    P = s.cam.proj_mat
    f = FakeFiller(s)
    alpha = np.random.default_rng(4).uniform(0, 1, T).astype(np.float32)
    alpha[:50], alpha[50:100] = 0.0, 1.0
    out = f.transparency_pass(alpha, layers=3, background=(1.0, 2.0, 3.0))
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (256, 256, 3)
    ground = (1.0, 2.0, 3.0)
    assert f.events == ["push", "settle", (BLEND, T, 1, True, None, ground), (NEXT, T, 0), (BLEND, T, 0, False, None, ground),
                        (NEXT, T, 0), (BLEND, T, 2, False, None, ground)]
    want = peel_ref.transparency(s.frags, s.tri, s.col, s.nrm, P, alpha, 3, background=ground, front=s.cam.color_buffer)
    assert_bit_equal(out.numpy(), want, "the model's plane")
    assert (want != s.cam.color_buffer).any()
    assert not f._host_fresh and not f._host_exposed
    assert_bit_equal(f.color_buffer.numpy(), s.cam.color_buffer, "the colour plane is only read")
    # the defaults; a number; the light; front="model"; one layer is FIRST | LAST
    sig = inspect.signature(DeferredPasses.transparency_pass)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == \
        [("alpha", inspect.Parameter.empty), ("layers", 4), ("light_direction", None), ("background", (0, 0, 0)),
         ("front", "plane")]
    f.events.clear()
    light = [float(v) for v in np.float32([0.6, 0.0, -0.8])]
    got = f.transparency_pass(0.5, light_direction=light, front="model")
    assert [e[0] for e in f.events[2:]] == [BLEND, NEXT, BLEND, NEXT, BLEND, NEXT, BLEND]
    assert f.events[2] == (BLEND, T, 1, False, tuple(light), (0.0, 0.0, 0.0)) and f.events[-1][2] == 2
    assert_bit_equal(got.numpy(), peel_ref.transparency(s.frags, s.tri, s.col, s.nrm, P, 0.5, 4, light=light), "with the light")
    f.events.clear()
    f.transparency_pass(torch.from_numpy(alpha), layers=1)
    assert f.events == ["push", "settle", (BLEND, T, 3, True, None, (0.0, 0.0, 0.0))]
    # alpha = 1 is the colour plane over the background
    got = f.transparency_pass(1.0, layers=2, background=(9.0, 8.0, 7.0)).numpy()
    want = s.cam.color_buffer.copy()
    want[~s.covered] = (9.0, 8.0, 7.0)
    assert_bit_equal(got, want, "alpha = 1")
    # an edit made in a view is carried up first and shows in front="plane"
    view = f.get_color_buffer()
    view[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    f.events.clear()
    got = f.transparency_pass(1.0, layers=1).numpy()
    assert f.events[0] == "push" and (got[100:140, 100:140][s.covered[100:140, 100:140]] == np.float32([10.0, 100.0, 200.0])).all()
    # a row strip fills its rows and leaves the others zero
    g = FakeFiller(s, row_strip=(37, 75))
    strip = g.transparency_pass(alpha, layers=3, background=ground).numpy()
    assert not strip[:37].any() and not strip[75:].any()
    want = peel_ref.transparency(s.frags, s.tri, s.col, s.nrm, P, alpha, 3, background=ground, front=s.cam.color_buffer,
                                 y0=37, y1=75)
    assert_bit_equal(strip, want, "the strip")


def test_the_methods_refuse_what_edge_aa_refuses_and_name_bad_arguments(soup71):
    s = soup71
    T = len(s.tri)
    for name, call in (("peel_layers", lambda f: f.peel_layers(2)), ("transparency_pass", lambda f: f.transparency_pass(0.5))):
        f = FakeFiller(s)
        f._pipeline = object()
        with pytest.raises(ValueError, match=name + r" is not available on a swap chain \(pipeline=True\)"):
            call(f)
        with pytest.raises(ValueError, match=name + " needs the winner plane"):
            call(FakeFiller(s, track_winner=False))
        f = FakeFiller(s)
        f._inputs = None
        with pytest.raises(ValueError, match=name + ": no frame has been rendered"):
            call(f)
        f = FakeFiller(s)
        f._last_flags = 0
        with pytest.raises(ValueError, match=name + ": the last frame did not start from cleared buffers"):
            call(f)
        assert f.events == []
    f = FakeFiller(s)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(ValueError, match="alpha must"):
            f.transparency_pass(bad)
    a = np.full(T, 0.5, np.float32)
    for i, bad in ((0, -1e-6), (7, 1.0001), (T - 1, np.nan)):
        b = a.copy()
        b[i] = bad
        with pytest.raises(ValueError, match=r"alpha must lie in \[0, 1\]: 1 of 3000 values do not"):
            f.transparency_pass(b)
    with pytest.raises(ValueError, match=f"alpha holds {T - 1} triangles, the last frame drew {T}"):
        f.transparency_pass(a[:-1])
    with pytest.raises(ValueError, match=f"alpha holds {T + 1} triangles, the last frame drew {T}"):
        f.transparency_pass(torch.zeros(T + 1))
    with pytest.raises(ValueError, match="alpha must be a number or float32"):
        f.transparency_pass(torch.zeros(T, dtype=torch.float64))
    with pytest.raises(ValueError, match="alpha must be a number or an array"):
        f.transparency_pass(np.zeros((T, 1), np.float32))
    for bad in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="layers must be an int from 1 to 16, got " + re.escape(repr(bad))):
            f.transparency_pass(0.5, layers=bad)
    for bad in ("colour", None, 0):
        with pytest.raises(ValueError, match="front must be 'plane' or 'model', got " + re.escape(repr(bad))):
            f.transparency_pass(0.5, front=bad)
    for bad in ((0, 0), (0, 0, float("nan")), 5, "abc", (0, 0, 1e39)):
        with pytest.raises(ValueError, match="background must be three finite numbers"):
            f.transparency_pass(0.5, background=bad)
        with pytest.raises(ValueError, match="light_direction must be None or three finite numbers"):
            f.transparency_pass(0.5, light_direction=bad)
    assert f.events == []                                                 # nothing was pushed, settled or launched
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    assert AdvancedPixelBufferFiller.transparency_pass is DeferredPasses.transparency_pass
    assert AdvancedPixelBufferFiller.peel_layers is DeferredPasses.peel_layers


# ---- the Renderer ----------------------------------------------------------------------------------------------

# a filler that records what the Renderer asks of it; ``image`` is what its pass returns
IMAGE = torch.arange(8 * 8 * 3, dtype=torch.float32).reshape(8, 8, 3)
_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass phong_pass shade_guro get_color_tensor get_color_buffer transparency_pass",
    returns=dict(transparency_pass=IMAGE), quiet="_push_host_edits synchronize get_normals_buffer", image=IMAGE)


def test_renderer_construction():
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    names = list(inspect.signature(Renderer.__init__).parameters)
    assert names[-3:] == ["transparency", "wireframe", "supersample"]
    assert inspect.signature(Renderer.__init__).parameters["transparency"].default is None
    assert Renderer(SimpleNamespace(), None).transparency is None

    class Plain:
        pass

    class Glass:
        def transparency_pass(self, alpha, layers=4, light_direction=None, background=(0, 0, 0), front="plane"):
            pass

        def phong_pass(self, *a, **kw):
            pass

        def edge_aa(self, edges=None):
            pass

        def depth_of_field(self, focus):
            pass

        def resolve(self, s):
            pass
    with pytest.raises(ValueError, match=r"Renderer\(transparency=\.\.\.\) needs a filler with a transparency pass.*Plain has no transparency_pass"):
        Renderer(Plain(), None, transparency=dict(alpha=0.5))
    for other in (dict(antialias={}), dict(depth_of_field=dict(focus=1.0)), dict(supersample=2)):
        with pytest.raises(ValueError, match="transparency.*antialias.*depth_of_field.*supersample.*reads the filler's own colour plane"):
            Renderer(Glass(), None, transparency=dict(alpha=0.5), **other)
    with pytest.raises(ValueError, match=r"Renderer\(transparency=\.\.\.\) with a PhongIllumination"):
        Renderer(Glass(), PhongIllumination(position=(0.0, 0.0, 1.0)), transparency=dict(alpha=0.5))
    with pytest.raises(ValueError, match=r"\['opacity'\] unknown"):
        Renderer(Glass(), None, transparency=dict(alpha=0.5, opacity=2))
    with pytest.raises(ValueError, match="needs 'alpha'"):
        Renderer(Glass(), None, transparency={})
    opts = dict(alpha=0.25, layers=6, background=(1, 2, 3), front="model")
    r = Renderer(Glass(), None, transparency=opts)
    assert r.transparency == opts and r.transparency is not opts
    assert Renderer(Glass(), None, antialias={}).transparency is None


def test_renderer_runs_the_pass_last_and_returns_its_plane():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    model = SimpleNamespace(_vertices_by_triangles=np.zeros((1, 3, 3), np.float32))
    guro = GuroIllumination(LIGHT)
    alpha = torch.full((1,), 0.5)
    opts = dict(alpha=alpha, layers=3)
    # fused: a cleared frame, the pass last with the illumination's light, its tensor handed out
    f = _Recorder()
    r = Renderer(f, guro, on_device="fused", transparency=opts)
    assert r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "get_color_tensor", "transparency_pass"]
    assert f.calls[1][2].get("clear") is True
    kw = f.calls[-1][2]
    assert kw["alpha"] is alpha and kw["layers"] == 3 and kw["light_direction"] is guro.light_direction and len(kw) == 3
    # on the device, after the light and after the wire pass, every frame
    f = _Recorder()
    r = Renderer(f, guro, on_device=True, wireframe=dict(width=2.0), transparency=opts)
    assert r.render(model) is f.image and r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "shade_guro", "wire_pass", "get_color_tensor",
                                       "transparency_pass"] * 2
    assert all(c[2].get("clear") is True for c in f.calls if c[0] == "render_model")
    # None and False return a fresh numpy copy of the pass's plane; a numpy alpha goes through as it is
    a = np.float32([0.5])
    for on_device in (None, False):
        f = _Recorder()
        got = Renderer(f, guro, on_device=on_device, transparency=dict(alpha=a)).render(model)
        assert isinstance(got, np.ndarray) and np.array_equal(got, f.image.numpy())
        assert f.calls[-1][0] == "transparency_pass" and f.calls[-1][2]["alpha"] is a
        assert [c[0] for c in f.calls].count("transparency_pass") == 1
        assert all(c[2].get("clear") is True for c in f.calls if c[0] == "render_model")
    # an illumination without a light direction: the layers behind are unlit; an explicit key wins
    f = _Recorder()
    flat = SimpleNamespace(draw_illumination=lambda colour, normals: None)
    Renderer(f, flat, transparency=dict(alpha=0.5)).render(model)
    assert f.calls[-1][0] == "transparency_pass" and f.calls[-1][2]["light_direction"] is None
    f = _Recorder()
    Renderer(f, guro, on_device="fused", transparency=dict(alpha=0.5, light_direction=(0, 0, -1))).render(model)
    assert f.calls[-1][2]["light_direction"] == (0, 0, -1)
    # without the option nothing changes: no pass, the filler's own colours
    f = _Recorder()
    assert Renderer(f, guro, on_device="fused").render(model) == "colour"
    assert "transparency_pass" not in [c[0] for c in f.calls] and f.calls[1][2] == dict(clear=True)
