"""The outline without a GPU: the header against the binding and the library, the entry point's argument checks, the
host model the GPU tests compare with (tests/outline_ref.py) pinned on the oracle's frames by counts, by identities, on
a hand-built scene of two triangles and against a float64 evaluation, ``wire_pass``'s new argument checks and
``Renderer(wireframe={"outline": True, ...})``."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import outline_ref
import overlay_ref
import tex_ref
from pass_scenes import Frame, capi, recording_filler, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from util import assert_bit_equal, other_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTLINE_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_float), C.c_void_p,
                    C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p,
                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p]


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_outline_symbol_is_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_wire.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert "crender_wire_outline" in declared and declared == set(capi.UNIT_SIGNATURES["wire"])
    assert not declared & other_symbols(capi, "wire")
    res, args = capi.UNIT_SIGNATURES["wire"]["crender_wire_outline"]
    assert res == C.c_int and args == OUTLINE_ARGTYPES
    assert capi.load().crender_wire_outline.argtypes == OUTLINE_ARGTYPES
    decl = re.search(r"CRENDER_API int crender_wire_outline\((.*?)\);", header, re.S).group(1)
    params = [" ".join(a.split()) for a in decl.split(",")]
    assert len(params) == len(args) == 21
    assert params == ["const int32_t *d_winner", "const float *d_z", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of",
                      "const float *P16", "const uint8_t *d_edges", "const float *line3", "const float *fill3", "float width",
                      "float feather", "float opacity", "float depth_bias", "int radius_px", "float *d_color", "int H", "int W",
                      "int y0", "int y1", "unsigned flags", "void *stream"]
    floats = [i for i, a in enumerate(params) if re.match(r"float \w+$", a)]
    assert floats == [i for i, a in enumerate(args) if a is C.c_float] == [9, 10, 11, 12]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert "crender_wire_outline" in set(re.findall(r" T (crender_\w+)", out))
    limits = dict(re.findall(r"#define (CRENDER_WIRE_\w+) (\d+)", header))
    assert int(limits["CRENDER_WIRE_OUTLINE_MAX_RADIUS"]) == capi.WIRE_OUTLINE_MAX_RADIUS == outline_ref.MAX_RADIUS == 8
    assert int(limits["CRENDER_WIRE_MAX_WIDTH"]) == outline_ref.MAX_WIDTH
    assert capi.ABI_VERSION == 6


def test_outline_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    nan, inf = float("nan"), float("inf")
    white = (C.c_float * 3)(255.0, 255.0, 255.0)
    grey = (C.c_float * 3)(40.0, 40.0, 40.0)

    def outline(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=P, edges=None, line=white, fill=None, width=1.0, feather=1.0,
                opacity=1.0, bias=1e-3, radius=2, col=fake, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_wire_outline(win, z, tri, T, pos_of, P, edges, line, fill, width, feather, opacity, bias, radius, col,
                                      H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(z=None), dict(P=None), dict(line=None), dict(col=None)):
        assert outline(**kw) == E and "is NULL" in text(), kw
    assert outline(tri=None) == E and "NULL with T > 0" in text()
    assert outline(T=-1) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2)):
        assert outline(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert outline(**kw) == E and "rows outside the frame" in text(), kw
    for name in ("width", "feather"):
        for bad in (nan, inf, -inf, 0.0, -1.0, 64.5, 1e30):
            assert outline(**{name: bad}) == E and f"{name} is not in (0, 64]" in text(), (name, bad)
    for bad in (nan, inf, -inf, -0.001, 1.001):
        assert outline(opacity=bad) == E and "opacity is not in [0, 1]" in text(), bad
    for bad in (nan, inf, -inf):
        assert outline(bias=bad) == E and "depth_bias is not finite" in text(), bad
    for bad in (-1, 9, 32, -2 ** 31, 2 ** 31 - 1):
        assert outline(radius=bad) == E and "radius_px is not 0 .. 8" in text(), bad
    for bad in (nan, inf, -inf):
        for i in range(3):
            c = [255.0] * 3
            c[i] = bad
            assert outline(line=(C.c_float * 3)(*c)) == E and "not finite" in text(), (bad, i)
            assert outline(fill=(C.c_float * 3)(*c)) == E and "not finite" in text(), (bad, i)
    for flags in (1, 2, 0x80000000):
        assert outline(flags=flags) == E and "unknown flag bits" in text(), flags
    assert text().startswith("crender_wire_outline")
    # the ends of the ranges are inside; without triangles there is nothing to launch
    assert outline(T=0, tri=None) == capi.OK
    assert outline(T=0, width=64.0, feather=64.0, opacity=0.0, fill=grey, edges=fake, radius=8, bias=-1e30) == capi.OK
    assert outline(T=0, width=1e-30, feather=1e-30, radius=0, bias=0.0) == capi.OK
    assert outline(T=0, radius=9) == E


# ---- the model on the oracle's frames --------------------------------------------------------------------------

class _Frame(Frame):
    def run(self, **kw):
        return outline_ref.wire_pass(self.cam.color_buffer, self.cam.winner, self.cam.z_buffer, self.tri, self.cam.proj_mat, **kw)

    def distances(self, **kw):
        return outline_ref.distances(self.cam.winner, self.cam.z_buffer, self.tri, self.cam.proj_mat, **kw)


SOUPS = {51: (4000, 200, 173, (1.0, 40.0)), 71: (3000, 256, 256, (3.0, 50.0))}       # test_wire_pass_cpu.py's scenes


soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)


def test_the_counts_on_trex(trex):
    """T-Rex at 256^2, feather 1, the default radius (2 at width 1, 3 at width 3) and bias.  (The overlay, outline=False, reaches 14 275 covered
    pixels with all edges at width 1 and 3 145 under the mask, and no background pixel: tests/test_wire_pass_cpu.py.)"""
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    mask = feature_edges(trex.tri, 30.0)
    want = {("all", 1.0): dict(covered=15801, background_on=848, covered_on=14292, full=0, partial=15140, nan=0),
            ("all", 3.0): dict(covered=15801, background_on=1684, covered_on=15731, full=15142, partial=2273, nan=0),
            ("feature", 1.0): dict(covered=15801, background_on=583, covered_on=4250, full=0, partial=4833, nan=0),
            ("feature", 3.0): dict(covered=15801, background_on=1264, covered_on=6739, full=4847, partial=3156, nan=0)}
    for (name, width), counts in want.items():
        edges = None if name == "all" else mask
        c = {}
        out = trex.run(edges=edges, width=width, counts=c)
        assert c == counts, (name, width, c)
        assert c["background_on"] > 0 and not np.isnan(out).any()
    # the background is written on a line only, also under a fill
    out = trex.run(edges=mask, width=3.0, fill=(1.0, 2.0, 3.0), counts=c)
    changed = (out.view(np.uint32) != trex.cam.color_buffer.view(np.uint32)).any(2)
    assert int((changed & ~trex.covered).sum()) == c["background_on"] == 1264
    assert not (out[~trex.covered] == np.float32([1.0, 2.0, 3.0])).all(1).any()


@pytest.mark.parametrize("seed,measured", [(51, 1.13e-5), (71, 1.56e-5)])
def test_the_distances_against_float64(soups, seed, measured):
    """The same statements from the same float32 projected corners in float64, no pixel excluded, all edges, radius 2
    (the default at width 1 and feather 1) and the default bias.  Measured with this model: the largest |m - m64| is
    1.120e-5 pixels on seed 51 and 1.556e-5 on seed 71 (the closest point is formed from corners up to a few hundred
    pixels from the pixel, then subtracted from it: one float32 rounding of each product and sum).  The bound is four
    times the measured value, as in test_wire_pass_cpu.py: the margin is for other frames of the same scale.  It is a
    check of the model's statements, not a bound on the kernel, which is held to bit equality with the float32 model.
    The depth test is a decision, not a rounding: where (ze - depth_bias) < z falls the other way in float64 another
    edge is the nearest.  At radius 2 no pixel of these frames decides differently; at radius 3 one pixel of seed 51
    does and is 0.74 pixels off, which is why the radius is pinned here."""
    f = soups[seed]
    (m32, _, _), (m64, _, _) = f.distances(radius_px=2), f.distances(radius_px=2, dtype=np.float64)
    assert m32.dtype == np.float32 and m64.dtype == np.float64 and not np.isnan(m64).any()
    assert (np.isinf(m32) == np.isinf(m64)).all()
    both = np.isfinite(m64)
    diff = float(np.abs(m32.astype(np.float64)[both] - m64[both]).max())
    print(f"seed {seed}: largest |m - m64| = {diff:.3e} pixels (bound {4 * measured:.3e})")
    assert 0 < diff <= 4 * measured


def test_identities(soups, trex):
    f = soups[71]
    base = f.cam.color_buffer
    T = len(f.tri)
    fill = (10.0, 20.0, 30.0)
    mask = np.random.default_rng(5).integers(0, 8, T).astype(np.uint8)
    # per pixel, m never grows with the radius: the minimum runs over a superset
    fields = [f.distances(edges=mask, radius_px=r)[0] for r in (0, 1, 2, 4, 8)]
    for near, far in zip(fields, fields[1:]):
        assert (far <= near).all() and (far < near).any()
    # radius 0 is the model restricted to the own winner: the background sees nothing, and a covered pixel the segments
    # of its own triangle, never nearer than the overlay's lines through them
    m0, own, _ = f.distances(edges=mask, radius_px=0)
    assert np.isinf(m0[own < 0]).all() and (own >= 0).sum() == f.covered.sum()
    ys, xs, t, line, _ = overlay_ref.distances(f.cam.winner, f.tri, f.cam.proj_mat, mask)
    assert (m0[ys, xs] >= line - np.float32(1e-3)).all() and (m0[ys, xs] > line + 1).any()
    restricted = np.full(f.cam.winner.shape, np.inf, np.float32)
    for tt in np.unique(t)[:200]:                  # one triangle at a time: a plane that holds that winner alone
        alone = np.where(f.cam.winner == tt, f.cam.winner, -1)
        one = outline_ref.distances(alone, f.cam.z_buffer, f.tri, f.cam.proj_mat, mask, radius_px=0)[0]
        at = f.cam.winner == tt
        restricted[at] = one[at]
        assert_bit_equal(one[at], m0[at], f"triangle {tt} alone")
    # a background-only frame and T = 0 change nothing
    nothing = np.full_like(f.cam.winner, -1)
    for kw in (dict(), dict(fill=fill)):
        out = outline_ref.wire_pass(base, nothing, f.cam.z_buffer, f.tri, f.cam.proj_mat, width=3.0, radius_px=8, **kw)
        assert_bit_equal(out, base, "a background-only frame")
        out = outline_ref.wire_pass(base, f.cam.winner, f.cam.z_buffer, f.tri[:0], f.cam.proj_mat, width=3.0, **kw)
        assert_bit_equal(out, base, "T = 0")
    # rows outside [y0, y1) are neither read nor written: poisoned winners, colours and depths there change nothing
    y0, y1 = 40, 136
    strip = f.run(width=3.0, edges=mask, fill=fill, y0=y0, y1=y1)
    assert_bit_equal(strip[:y0], base[:y0], "rows above the strip")
    assert_bit_equal(strip[y1:], base[y1:], "rows below the strip")
    winner, z, color = f.cam.winner.copy(), f.cam.z_buffer.copy(), base.copy()
    winner[:y0], winner[y1:] = 0, 1
    z[:y0], z[y1:] = -5.0, np.nan
    color[:y0], color[y1:] = 7.5, -2.25
    poisoned = outline_ref.wire_pass(color, winner, z, f.tri, f.cam.proj_mat, width=3.0, edges=mask, fill=fill, y0=y0, y1=y1)
    assert_bit_equal(poisoned[y0:y1], strip[y0:y1], "the strip does not see across its edge")
    assert (poisoned[:y0] == 7.5).all() and (poisoned[y1:] == -2.25).all()
    whole = f.run(width=3.0, edges=mask, fill=fill)
    assert (whole[y0:y1] != strip[y0:y1]).any() and (whole[y0 + 8:y1 - 8] == strip[y0 + 8:y1 - 8]).all()
    # with a fill a covered pixel that is off equals the fill
    c = {}
    out = f.run(width=1.0, edges=mask, fill=fill, counts=c)
    m, own, _ = f.distances(edges=mask, radius_px=2)
    off = (own >= 0) & ~((np.float32(1.0) - m) / np.float32(1.0) > 0)
    assert int(off.sum()) == c["covered"] - c["covered_on"] > 1000
    assert (out[off] == np.float32(fill)).all()
    # no edge drawn: nothing without a fill, the fill on every covered pixel with it; bits 3 to 7 are ignored
    none = np.zeros(T, np.uint8)
    assert_bit_equal(f.run(edges=none, width=3.0), base, "no edge drawn")
    out = f.run(edges=np.full(T, 0xF8, np.uint8), fill=fill)
    assert (out[f.covered] == np.float32(fill)).all()
    assert_bit_equal(out[~f.covered], base[~f.covered], "the fill leaves the background alone")
    assert_bit_equal(f.run(edges=np.full(T, 0xFF, np.uint8)), f.run(), "all bits against no mask")
    # the style does not enter the distances: a field computed once serves every width
    field = trex.distances(radius_px=3)
    assert_bit_equal(trex.run(width=3.0, field=field), trex.run(width=3.0), "a field handed in")


# ---- two triangles, the near one over the far one ---------------------------------------------------------------

def _screen(oracle_P, pts, z, H, W):
    """Model-space corners that project to about the screen points `pts` at depth z."""
    f = float(oracle_P[0, 0])
    g = float(oracle_P[1, 1])
    pts = np.float64(pts)
    return np.stack([(pts[:, 0] / (W / 2.0) - 1.0) * z / f, (pts[:, 1] / (H / 2.0) - 1.0) * z / g, np.full(3, z)], 1).astype(np.float32)


def _segment64(a, b, xs, ys):
    """(distance, s unclamped) of the points to the segment a b, in float64."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    e = b[:2] - a[:2]
    s = ((xs - a[0]) * e[0] + (ys - a[1]) * e[1]) / (e @ e)
    sc = np.clip(s, 0, 1)
    return np.hypot(xs - (a[0] + sc * e[0]), ys - (a[1] + sc * e[1])), s


@pytest.mark.parametrize("bias", [0.0, 1e-3])
def test_a_near_triangle_over_a_far_one(oracle, bias):
    H = W = 64
    cam = oracle.OracleFiller(H, W, fov=45.0)
    P = cam.proj_mat
    far = _screen(P, [(4, 4), (36, 6), (8, 60)], 2.0, H, W)             # its edge 1 passes behind the near triangle
    near = _screen(P, [(20, 20), (50, 24), (30, 50)], 1.0, H, W)        # its right part lies over the background
    tri = np.ascontiguousarray(np.stack([far, near]))
    nrm = np.zeros((2, 3, 3), np.float32)
    nrm[..., 2] = -1.0
    cam.render_arrays(tri, np.full((2, 3, 3), 100.0, np.float32), nrm)
    win, z = cam.winner, cam.z_buffer
    assert (win == 0).sum() > 400 and (win == 1).sum() > 300 and (win < 0).sum() > 1000
    proj = tex_ref.project(tri, P, W, H)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    width, feather = 3.0, 1.0
    hi = (width + feather) / 2
    # float32 corners up to 64 px from a pixel: each of the dozen steps rounds by at most 2^-24 * 64 px
    tol = 12 * 64 * 2.0 ** -24
    for e in range(3):
        # edge e of the near triangle alone: a silhouette all along
        mask = np.uint8([0, 1 << e])
        m, own, _ = outline_ref.distances(win, z, tri, P, mask, radius_px=outline_ref.default_radius(width, feather), depth_bias=bias)
        d64, s = _segment64(proj[1, e], proj[1, (e + 1) % 3], xs, ys)
        interior = (s > 0.1) & (s < 0.9)
        inner, outer = interior & (win == 1), interior & (win != 1)
        on = (np.float32(hi) - m) / np.float32(feather) > 0
        want_on = d64 < hi - tol
        # the outer half: on at far-triangle pixels and at background pixels within the window
        assert (on[outer & want_on]).all() and not on[interior & (d64 > hi + tol)].any()
        for side, name in ((outer & (win == 0), "far"), (outer & (win < 0), "background"), (inner, "inner")):
            hit = side & want_on
            # (edge 1, from (50, 24) to (30, 50), lies over the background alone)
            assert hit.sum() >= (0 if (name, e) == ("far", 1) else 10), (e, name, int(hit.sum()))
            # and the profile across the silhouette is the same outside as inside: the distance to the segment
            assert np.abs(m[hit].astype(np.float64) - d64[hit]).max(initial=0.0) <= tol, (e, name)
    # the far triangle's edges alone: none is on at a near-triangle pixel, though its edge 1 passes right behind some
    mask = np.uint8([7, 0])
    m, own, _ = outline_ref.distances(win, z, tri, P, mask, radius_px=3, depth_bias=bias)
    d64 = _segment64(proj[0, 1], proj[0, 2], xs, ys)[0]
    behind = (win == 1) & (d64 < 1.0)
    assert behind.sum() >= 10
    assert np.isinf(m[win == 1]).all()
    assert np.isfinite(m[(win == 0) & (d64 < 1.0)]).all() and ((win == 0) & (d64 < 1.0)).sum() >= 10
    # all edges, as colours: a near pixel never shows a line that is not its own triangle's
    out = outline_ref.wire_pass(cam.color_buffer, win, z, tri, P, width=width, feather=feather, depth_bias=bias)
    alone = outline_ref.wire_pass(cam.color_buffer, np.where(win == 1, 1, -1).astype(np.int32), z, tri, P, width=width,
                                  feather=feather, depth_bias=bias)
    assert_bit_equal(out[win == 1], alone[win == 1], "the near triangle's pixels")


# ---- the Python layer ------------------------------------------------------------------------------------------

def test_wire_pass_refuses_bad_outline_arguments_before_it_looks_at_the_device():
    """The checks of the Python layer on a stand-in that has no device at all."""
    from cython3dmodelrenderer_amd import _capi
    from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses
    assert _capi.WIRE_OUTLINE_MAX_RADIUS == 8
    calls = []
    stub = SimpleNamespace(_pipeline=None, winner_buffer=object(), _inputs=(np.zeros((5, 3, 3), np.float32),), _last_flags=1,
                           device="cpu")
    stub._pass_target = lambda name: DeferredPasses._pass_target(stub, name)
    stub._pass_frame = lambda name, who=None: DeferredPasses._pass_frame(stub, name, who)
    stub._run_pass = lambda entry, tri, T, operands, flags=0, more=(), z=False, light=None: calls.append((entry, T, operands, z))

    def wire_pass(**kw):
        return DeferredPasses.wire_pass(stub, **kw)
    for kw, word in ((dict(radius_px=-1), "radius_px"), (dict(radius_px=9), "radius_px"), (dict(radius_px=2.5), "radius_px"),
                     (dict(radius_px="2"), "radius_px"), (dict(radius_px=True), "radius_px"),
                     (dict(depth_bias=float("nan")), "depth_bias"), (dict(depth_bias=float("inf")), "depth_bias"),
                     (dict(depth_bias=-float("inf")), "depth_bias"), (dict(depth_bias=None), "depth_bias"),
                     (dict(width=14.0, feather=0.5), "at most 14"), (dict(width=64.0), "at most 14"),
                     (dict(width=0), "width"), (dict(feather=float("inf")), "feather"), (dict(opacity=1.5), "opacity")):
        with pytest.raises(ValueError, match=word):
            wire_pass(outline=True, **kw)
    with pytest.raises(ValueError, match=r"T = 5.*\(4,\)"):
        wire_pass(outline=True, edges=np.zeros(4, np.uint8))
    assert not calls
    # what reaches the library: the overlay's call, bit for bit, without `outline`; the new entry with z and the two
    # operands behind the opacity with it
    wire_pass(width=2.0, radius_px=77, depth_bias=float("nan"))        # (both ignored without outline)
    wire_pass(width=2.0, outline=True)
    wire_pass(width=3.0, feather=0.5, outline=True, depth_bias=0, radius_px=np.int64(8))
    wire_pass(width=10.0, feather=4.0, outline=True, depth_bias=-2e-3)
    wire_pass(width=0.25, feather=0.25, outline=True, radius_px=0)
    (e0, T0, op0, z0), (e1, T1, op1, z1), (e2, _, op2, _), (e3, _, op3, _), (e4, _, op4, _) = calls
    assert (e0, T0, z0, len(op0)) == ("crender_wire_overlay", 5, False, 6) and op0[3:] == (2.0, 1.0, 1.0)
    assert (e1, T1, z1, len(op1)) == ("crender_wire_outline", 5, True, 8) and op1[3:] == (2.0, 1.0, 1.0, 1e-3, 3)
    assert e2 == e3 == e4 == "crender_wire_outline"
    assert op2[3:] == (3.0, 0.5, 1.0, 0.0, 8) and type(op2[7]) is int and type(op2[6]) is float
    assert op3[3:] == (10.0, 4.0, 1.0, -2e-3, 8) and op4[3:] == (0.25, 0.25, 1.0, 1e-3, 0)
    assert op1[0] is None and list(op1[1]) == [255.0, 255.0, 255.0] and op1[2] is None
    for width, feather, radius in ((1.0, 1.0, 2), (3.0, 1.0, 3), (3.0, 0.5, 3), (0.5, 0.25, 2), (13.0, 1.0, 8), (4.0, 2.0, 4)):
        assert outline_ref.default_radius(width, feather) == radius
        calls.clear()
        wire_pass(width=width, feather=feather, outline=True)
        assert calls[0][2][7] == radius
    chain = SimpleNamespace(**vars(stub))
    chain._pipeline = object()
    chain._pass_target = lambda name: DeferredPasses._pass_target(chain, name)
    with pytest.raises(ValueError, match="swap chain"):
        DeferredPasses.wire_pass(chain, outline=True)


# a filler that records what the Renderer asks of it
_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass phong_pass shadow_pass bind_shadow_map get_color_tensor resolve",
    returns=dict(resolve="resolved"))


def test_renderer_forwards_the_outline_options():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    import inspect
    from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses
    opts = dict(outline=True, depth_bias=2e-3, radius_px=4, width=2.0, fill=(1, 2, 3))
    # what the Renderer forwards, the real pass takes, with today's call as the default
    params = inspect.signature(DeferredPasses.wire_pass).parameters
    assert set(opts) <= set(params)
    assert (params["outline"].default, params["depth_bias"].default, params["radius_px"].default) == (False, 1e-3, None)
    model = SimpleNamespace()
    # the fused light: draw, then the lines
    f = _Recorder()
    r = Renderer(f, GuroIllumination((0.3, -0.2, 1.0)), on_device="fused", wireframe=opts)
    assert r.wireframe == opts and r.wireframe is not opts
    assert r.render(model) == "colour"
    names = [c[0] for c in f.calls]
    assert names.index("render_model") < names.index("wire_pass") < names.index("get_color_tensor")
    assert [c[2] for c in f.calls if c[0] == "wire_pass"] == [opts]
    # supersampled: the lines before the resolve, which carries no light
    f = _Recorder(16, 16)
    r = Renderer(f, GuroIllumination((0.3, -0.2, 1.0)), None, 8, 8, on_device="fused", wireframe=opts, supersample=2)
    assert r.render(model) == "resolved"
    names = [c[0] for c in f.calls]
    assert names.index("render_model") < names.index("wire_pass") < names.index("resolve")
    assert [c for c in f.calls if c[0] == "wire_pass"] == [("wire_pass", (), opts)]
    assert [c for c in f.calls if c[0] == "resolve"] == [("resolve", (2,), {})]
    # a PhongIllumination, supersampled: the lines after the light and before the resolve
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    f = _Recorder(16, 16)
    r = Renderer(f, PhongIllumination(position=(0.0, 0.0, 1.0)), None, 8, 8, on_device=True, wireframe=opts, supersample=2)
    assert r.render(model) == "resolved"
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "phong_pass", "wire_pass", "resolve"]
    assert f.calls[3] == ("wire_pass", (), opts)
