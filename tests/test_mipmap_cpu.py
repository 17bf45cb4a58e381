"""Mipmaps and trilinear filtering without a GPU: the host model the GPU tests compare with (tests/mip_ref.py)
pinned on hand-made chains, a quad of known footprint, a constant texture, the magnified part of a frame and the
level histograms of T-Rex; the C ABI's exports, its host-only layout call and its argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mip_ref
import tex_ref
from pass_scenes import capi, texture, trex_uv as trex  # noqa: F401 (fixtures)
from util import INCLUDE, assert_bit_equal, other_symbols, unit_in_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 7), (2, 5), (3, 1000), (709, 709), (64, 97), (1025, 513)]


@pytest.fixture(scope="module")
def frames(oracle, trex):
    """The oracle's T-Rex frame per size, rendered once."""
    tri, col, nrm, _ = trex
    made = {}

    def frame(size):
        if size not in made:
            made[size] = oracle.OracleFiller(size, size, fov=45.0)
            made[size].render_arrays(tri, col, nrm)
        return made[size]
    return frame


def _c_layout(capi, th, tw):
    n = capi.MIP_MAX_LEVELS
    levels, total = C.c_int32(-1), C.c_uint64(0)
    hs, ws, offs = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_uint64 * n)()
    rc = capi.load().crender_mip_layout(th, tw, C.byref(levels), hs, ws, offs, C.byref(total))
    return rc, levels.value, list(hs), list(ws), list(offs), total.value


# ---- the host side of the ABI ----------------------------------------------------------------------------------

@pytest.mark.parametrize("th,tw", SIZES)
def test_layout_agrees_with_the_host_model(capi, th, tw):
    levels, offsets, total = mip_ref.layout(th, tw)
    rc, L, hs, ws, offs, got_total = _c_layout(capi, th, tw)
    assert rc == capi.OK
    assert L == len(levels) == 1 + int(np.floor(np.log2(max(th, tw))))
    assert list(zip(hs[:L], ws[:L])) == levels and offs[:L] == offsets and got_total == total
    assert not any(hs[L:]) and not any(ws[L:]) and not any(offs[L:])
    assert levels[0] == (th, tw) and levels[-1] == (1, 1)
    assert total == 3 * sum(h * w for h, w in levels)


def test_layout_refuses_an_empty_side_and_a_seventeenth_level(capi):
    L = capi.load()
    for th, tw in ((0, 4), (4, 0), (-1, 4), (65536, 1), (1, 65536)):
        assert _c_layout(capi, th, tw)[0] == capi.EINVAL, (th, tw)
        assert b"crender_mip_layout" in L.crender_last_error()
    rc, levels = _c_layout(capi, 65535, 65535)[:2]
    assert rc == capi.OK and levels == 16
    assert L.crender_mip_layout(709, 709, None, None, None, None, None) == capi.OK      # every output is optional
    for bad in ((0, 4), (65536, 1)):
        with pytest.raises(ValueError):
            mip_ref.layout(*bad)


def test_mip_header_symbols_are_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_mip.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["mip"]) == {"crender_mip_layout", "crender_mip_build", "crender_mip_shade"}
    assert not declared & other_symbols(capi, "mip")
    L = capi.load()
    for name in declared:
        assert getattr(L, name).argtypes == capi.UNIT_SIGNATURES["mip"][name][1]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    assert re.search(rf"\bCRENDER_MIP_PERSPECTIVE = {capi.MIP_PERSPECTIVE}u\b", header)
    assert re.search(rf"\bCRENDER_MIP_MAX_LEVELS = {capi.MIP_MAX_LEVELS}\b", header)
    # the shade entry point takes crender_tex_shade's arguments
    assert capi.UNIT_SIGNATURES["mip"]["crender_mip_shade"] == capi.UNIT_SIGNATURES["tex"]["crender_tex_shade"]


def test_mip_sources_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit_in_build(_build, "mip", ["texmip.hip"], [os.path.join(INCLUDE, "crender_mip.h"), "mip_sample.h"])
    others = _build.UNITS["wire"][0] + _build.UNITS["py"][0] + _build.UNITS["tex"][0] + _build.UNITS["wire"][1] + \
        _build.UNITS["py"][1] + _build.UNITS["tex"][1]
    assert not set(_build.UNITS["mip"][0] + _build.UNITS["mip"][1]) & set(others)


def test_mip_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    light = (C.c_float * 3)(0, 0, -1)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first

    def shade(win=fake, tri=fake, T=1, pos=None, P=P, uv=fake, chain=fake, th=4, tw=4, nrm=None, light=None, col=fake,
              H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_mip_shade(win, tri, T, pos, P, uv, chain, th, tw, nrm, light, col, H, W, y0, y1, flags, None)

    assert shade(win=None) == E and shade(tri=None) == E and shade(P=None) == E and shade(uv=None) == E
    assert shade(chain=None) == E and shade(col=None) == E
    assert shade(T=-1) == E
    assert shade(th=0) == E and shade(tw=0) == E and shade(th=-2) == E
    assert shade(th=65536) == E and shade(tw=65536) == E                 # a seventeenth level
    assert shade(H=0) == E and shade(W=-1) == E
    assert shade(y0=-1) == E and shade(y1=9) == E and shade(y0=4, y1=4) == E and shade(y0=5, y1=3) == E
    assert shade(light=light) == E                                       # a light without normals
    assert shade(nrm=fake) == E                                          # normals without a light
    assert shade(flags=2) == E and shade(flags=4) == E and shade(flags=0x80000001) == E     # unknown flag bits
    assert b"crender_mip_shade" in L.crender_last_error()
    # an empty scene without a light is no work at all: nothing is launched
    assert shade(T=0, tri=None, uv=None) == capi.OK
    assert L.crender_mip_build(None, 4, 4, fake, None) == E and L.crender_mip_build(fake, 4, 4, None, None) == E
    assert L.crender_mip_build(fake, 0, 4, fake, None) == E and L.crender_mip_build(fake, 4, 65536, fake, None) == E
    assert b"crender_mip_build" in L.crender_last_error()


def test_filler_and_renderer_carry_the_option():
    import inspect
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    sig = inspect.signature(AdvancedPixelBufferFiller.bind_texture)
    assert list(sig.parameters)[1:] == ["uv_by_triangles", "texture", "mipmaps"]
    assert sig.parameters["mipmaps"].default is False
    assert callable(AdvancedPixelBufferFiller.mip_levels) and callable(AdvancedPixelBufferFiller.get_mip_level)


# ---- the chain ---------------------------------------------------------------------------------------------------

def test_chain_properties():
    for th, tw in SIZES:
        tex = texture(th * 1000 + tw, th, tw)
        chain = mip_ref.build_chain(tex)
        levels, offsets, total = mip_ref.layout(th, tw)
        assert [c.shape for c in chain] == [(h, w, 3) for h, w in levels]
        assert np.array_equal(chain[0], tex)
        packed = mip_ref.pack_chain(chain)
        assert packed.dtype == np.uint8 and packed.size == total
        for c, at in zip(chain, offsets):
            assert np.array_equal(packed[at:at + c.size], c.reshape(-1))
    # (0 + 1 + 2 + 4 + 2) >> 2 = 2: rounded to nearest, halves up
    tiny = np.repeat(np.array([[0, 1], [2, 4]], np.uint8)[:, :, None], 3, axis=2)
    chain = mip_ref.build_chain(tiny)
    assert len(chain) == 2 and chain[1].tolist() == [[[2, 2, 2]]]
    assert mip_ref.build_chain(np.full((2, 2, 3), 255, np.uint8))[1].tolist() == [[[255, 255, 255]]]
    # constant on aligned 2^k blocks: level k holds those constants
    rng = np.random.default_rng(4)
    for k in (1, 2, 3):
        coarse = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
        tex = np.repeat(np.repeat(coarse, 1 << k, axis=0), 1 << k, axis=1)
        assert np.array_equal(mip_ref.build_chain(tex)[k], coarse), k
    # a 1 x N texture halves along N only, and an odd side clamps its last column
    row = rng.integers(0, 256, (1, 13, 3), dtype=np.uint8)
    chain = mip_ref.build_chain(row)
    assert [c.shape[:2] for c in chain] == [(1, 13), (1, 6), (1, 3), (1, 1)]
    want = (row[0, 0:12:2].astype(int) + row[0, 1:13:2] + 1) >> 1          # (2a + 2b + 2) >> 2
    assert np.array_equal(chain[1][0], want)
    three = np.array([[[10, 20, 30], [50, 60, 70], [200, 100, 0]]], np.uint8)
    assert mip_ref.build_chain(three)[1].tolist() == [[[30, 40, 50]]]      # column 2 is never read: w_1 = 1


def test_level_rule_by_hand():
    rho = np.float32([0.0, 0.5, 1.0, np.nan, 1.0000001, 1.5, 2.0, 3.0, 4.0, 7.0, 255.9, 256.0, 1e9, np.inf])
    l0, f = mip_ref.level_and_weight(rho, 9)
    assert l0.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 7, 8, 8, 8]
    assert_bit_equal(f, np.float32([0, 0, 0, 0, np.float32(1.0000001) - np.float32(1), 0.5, 0, 0.5, 0, 0.75,
                                    np.float32(255.9) / np.float32(128) - np.float32(1), 0, 0, 0]), "f")
    l0, f = mip_ref.level_and_weight(rho, 1)                 # a 1 x 1 texture: level 0, whatever the footprint
    assert not l0.any() and not f.any()
    assert l0.dtype == np.int32 and f.dtype == np.float32


# ---- the pass ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("perspective", [False, True])
def test_magnified_pixels_are_the_bilinear_ones(trex, frames, perspective):
    tri, _, _, uv = trex
    f = frames(1024)
    tex = texture(1, 709, 709)
    base = np.zeros((1024, 1024, 3), np.float32)
    got = mip_ref.texture_pass(base, f.winner, tri, f.proj_mat, uv, tex, perspective=perspective)
    ys, xs, u, v, rho, l0, w = mip_ref.pixel_levels(f.winner, tri, f.proj_mat, uv, 709, 709, perspective)
    magnified = ~(rho > 1)
    print(f"trex1024, perspective={perspective}: {int(magnified.sum())} of {len(ys)} covered pixels are magnified")
    assert len(ys) == 252539 and magnified.sum() >= 100000
    assert not l0[magnified].any() and not w[magnified].any()
    want = tex_ref.bilinear(u[magnified], v[magnified], tex)
    assert_bit_equal(got[ys[magnified], xs[magnified]], want, "magnified pixels")
    # and the frame as a whole is not the bilinear one
    plain = tex_ref.texture_pass(base, f.winner, tri, f.proj_mat, uv, tex, perspective=perspective, bilinear_filter=True)
    assert (plain[ys[~magnified], xs[~magnified]] != got[ys[~magnified], xs[~magnified]]).any()
    assert_bit_equal(got[f.winner < 0], base[f.winner < 0], "background")


def _screen_parallel_quad(oracle, H, W, th, tw, step_x, step_y):
    """Two triangles at constant z whose uv step `step_x` texels per pixel along x and `step_y` along y."""
    z = 2.0
    corners = np.array([[-0.31, -0.27, z], [0.33, -0.27, z], [0.33, 0.29, z], [-0.31, 0.29, z]], np.float32)
    tri = np.ascontiguousarray(corners[[[0, 1, 2], [0, 2, 3]]])
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1.0
    f = oracle.OracleFiller(H, W, fov=45.0)
    f.render_arrays(tri, np.full_like(tri, 255.0), nrm)
    proj = tex_ref.project(tri, f.proj_mat, W, H).astype(np.float64)
    X, Y = proj[..., 0], proj[..., 1]
    uv = np.stack([(X - X.min()) * step_x / tw, (Y - Y.min()) * step_y / th], axis=-1).astype(np.float32)
    return f, tri, uv, (X.min(), X.max(), Y.min(), Y.max())


@pytest.mark.parametrize("perspective", [False, True])
def test_a_quad_of_known_footprint_lands_halfway_between_levels_1_and_2(oracle, perspective):
    H = W = 256
    th = tw = 512
    f, tri, uv, (xl, xr, yt, yb) = _screen_parallel_quad(oracle, H, W, th, tw, 3.0, 1.25)
    ys, xs, u, v, rho, l0, w = mip_ref.pixel_levels(f.winner, tri, f.proj_mat, uv, th, tw, perspective)
    well_inside = (xs >= xl + 2) & (xs <= xr - 2) & (ys >= yt + 2) & (ys <= yb - 2)
    assert well_inside.sum() > 3000 and len(np.unique(f.winner[ys[well_inside], xs[well_inside]])) == 2
    # rho = 3 texels per pixel = 1.5 * 2^1: level 1, f = 0.5.  The bound is derived, not measured: u and v are of
    # order 1 and carry a handful of float32 roundings each (a few 1e-7); their differences, scaled by 512 texels,
    # are off by at most about 2e-4 texels, f = rho / 2 - 1 by half of that
    assert (l0[well_inside] == 1).all()
    err = float(np.abs(w[well_inside] - 0.5).max())
    print(f"quad, perspective={perspective}: max |f - 0.5| = {err:.3e} over {int(well_inside.sum())} pixels")
    assert err < 1e-3


def test_a_texture_of_one_colour_stays_that_colour(trex, frames):
    tri, _, _, uv = trex
    f = frames(256)
    colour = np.array([17, 200, 255], np.uint8)
    tex = np.broadcast_to(colour, (709, 709, 3)).copy()
    for perspective in (False, True):
        got = mip_ref.texture_pass(np.zeros((256, 256, 3), np.float32), f.winner, tri, f.proj_mat, uv, tex,
                                   perspective=perspective)
        covered = f.winner >= 0
        # about six roundings (two bilinear samples and their blend) on values <= 255, half an ulp of 1.5e-5 each
        err = float(np.abs(got[covered] - colour.astype(np.float32)).max())
        print(f"constant texture, perspective={perspective}: max error {err:.3e}")
        assert err < 1e-3
        assert not got[~covered].any()


@pytest.mark.parametrize("size,perspective,want", [
    (256, False, [233, 9591, 5004, 806, 121, 36, 9, 1, 0, 0]),
    (128, False, [0, 57, 2404, 1255, 196, 30, 13, 3, 0, 0]),
    (256, True, [231, 9588, 5006, 808, 124, 32, 11, 0, 1, 0]),
])
def test_level_histograms_of_trex(trex, frames, size, perspective, want):
    tri, _, _, uv = trex
    f = frames(size)
    _, _, _, _, rho, l0, w = mip_ref.pixel_levels(f.winner, tri, f.proj_mat, uv, 709, 709, perspective)
    got = np.bincount(l0, minlength=10).tolist()
    print(f"trex{size}, perspective={perspective}: levels {got}, {int((rho > 1).sum())} minified, "
          f"{int((rho > 2).sum())} beyond two texels per pixel")
    assert got == want
    assert (w >= 0).all() and (w < 1).all()
