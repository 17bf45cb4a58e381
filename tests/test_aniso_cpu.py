"""Anisotropic filtering without a GPU: the host model the GPU tests compare with (tests/aniso_ref.py) pinned by
hand — the sample offsets, the footprint rule on a table — and on the four consequences include/crender_aniso.h
states, over T-Rex and a receding floor; the C ABI's export, its argument checks, and the Python keyword."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import aniso_ref
import mip_ref
from pass_scenes import capi, trex_textured  # noqa: F401 (fixtures)
from util import INCLUDE, assert_bit_equal, other_symbols, unit_in_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def scenes_(oracle):
    """name -> (oracle frame, tri, uv, texture, chain): T-Rex at 256^2 and the floor at 64^2, rendered once."""
    out = {}
    for name, size, (tri, col, nrm, uv), tex_side in (("trex256", 256, trex_textured(), 709),
                                                       ("floor64", 64, aniso_ref.floor_scene(), 256)):
        f = oracle.OracleFiller(size, size, fov=45.0)
        f.render_arrays(tri, col, nrm)
        tex = np.random.default_rng(1).integers(0, 256, (tex_side, tex_side, 3), dtype=np.uint8)
        out[name] = (f, tri, uv, tex, mip_ref.build_chain(tex))
    return out


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_aniso_header_symbol_is_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_aniso.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["aniso"]) == {"crender_aniso_shade"}
    assert not declared & other_symbols(capi, "aniso")
    L = capi.load()
    assert L.crender_aniso_shade.argtypes == capi.UNIT_SIGNATURES["aniso"]["crender_aniso_shade"][1]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    assert capi.ANISO_MAX == 16 and re.search(rf"\bCRENDER_ANISO_MAX = {capi.ANISO_MAX}\b", header)
    assert aniso_ref.MAX_ANISO == capi.ANISO_MAX
    # crender_mip_shade's arguments in its order up to and including flags, then max_aniso, then the stream
    mip = capi.UNIT_SIGNATURES["mip"]["crender_mip_shade"]
    res, args = capi.UNIT_SIGNATURES["aniso"]["crender_aniso_shade"]
    assert res == mip[0] and args == mip[1][:-1] + [C.c_int, mip[1][-1]]
    assert capi.ABI_VERSION == 6


def test_aniso_sources_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit_in_build(_build, "aniso", ["texaniso.hip"], [os.path.join(INCLUDE, "crender_aniso.h"), "mip_sample.h"])
    assert _build.UNITS["mip"][0] == ["texmip.hip"]
    assert not any("mip" in name for name in _build.SOURCES + _build.HEADERS)
    # what the pass shares with texmip.hip is watched by both and by nothing else
    shared = set(_build.UNITS["aniso"][1]) & set(_build.UNITS["mip"][1])
    assert shared == {"mip_sample.h"}
    assert not shared & set(_build.UNITS["wire"][1] + _build.UNITS["py"][1] + _build.UNITS["tex"][1])


def test_aniso_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    light = (C.c_float * 3)(0, 0, -1)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first

    def shade(win=fake, tri=fake, T=1, pos=None, P=P, uv=fake, chain=fake, th=4, tw=4, nrm=None, light=None, col=fake,
              H=8, W=8, y0=0, y1=8, flags=0, A=4):
        return L.crender_aniso_shade(win, tri, T, pos, P, uv, chain, th, tw, nrm, light, col, H, W, y0, y1, flags, A,
                                     None)

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
    assert shade(A=0) == E and shade(A=-1) == E and shade(A=17) == E
    assert b"crender_aniso_shade" in L.crender_last_error()
    # an empty scene without a light is no work at all: nothing is launched
    for A in (1, 16):
        assert shade(T=0, tri=None, uv=None, A=A) == capi.OK
    assert shade(T=0, tri=None, uv=None, A=17) == E


def test_filler_carries_the_option_and_refuses_bad_values():
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    sig = inspect.signature(AdvancedPixelBufferFiller.texture_pass)
    assert list(sig.parameters)[1:] == ["perspective", "filter", "light_direction", "anisotropy"]
    assert sig.parameters["anisotropy"].default == 1
    assert list(inspect.signature(AdvancedPixelBufferFiller.bind_texture).parameters)[1:] == \
        ["uv_by_triangles", "texture", "mipmaps"]
    # the argument checks come before anything of the filler is looked at: no device is needed to see them
    nobody = types.SimpleNamespace()
    for bad in (0, 17, -1, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="anisotropy"):
            AdvancedPixelBufferFiller.texture_pass(nobody, filter="trilinear", anisotropy=bad)
    for filt in ("nearest", "bilinear"):
        with pytest.raises(ValueError, match='needs filter="trilinear"'):
            AdvancedPixelBufferFiller.texture_pass(nobody, filter=filt, anisotropy=4)
    with pytest.raises(ValueError, match="filter must be"):          # the filter's name is judged first
        AdvancedPixelBufferFiller.texture_pass(nobody, filter="anisotropic", anisotropy=0)
    sig = inspect.signature(aniso_ref.texture_pass)
    assert sig.parameters["anisotropy"].default == 1
    assert list(sig.parameters) == ["color", "winner", "tri", "P", "uv", "tex", "perspective", "anisotropy", "normals",
                                    "light_direction", "y0", "y1", "chain"]


# ---- the model by hand -------------------------------------------------------------------------------------------

def test_sample_offsets_by_hand():
    d = np.float32
    assert_bit_equal(aniso_ref.offsets(1), d([0.0]), "N = 1")
    assert_bit_equal(aniso_ref.offsets(2), d([-0.25, 0.25]), "N = 2")
    assert_bit_equal(aniso_ref.offsets(3), d([d(-2) / d(6), 0.0, d(2) / d(6)]), "N = 3")
    assert_bit_equal(aniso_ref.offsets(4), d([-0.375, -0.125, 0.125, 0.375]), "N = 4")
    for N in range(1, 17):
        o = aniso_ref.offsets(N)
        assert o.dtype == np.float32 and len(o) == N
        assert np.array_equal(o, -o[::-1]) and (np.abs(o) < 0.5).all()          # centred, inside the axis


def test_footprint_rule_by_hand():
    d = np.float32
    inf, nan = np.inf, np.nan
    table = [  # pmax, pmin, A -> rho, N
        (0.5, 0.1, 16, 0.5, 1),            # magnified: trilinear's rho, one sample
        (1.0, 0.2, 16, 1.0, 1),            # pmax <= 1 exactly
        (nan, 0.3, 4, nan, 1),             # a NaN major axis is "not minified"
        (8.0, nan, 4, 2.0, 4),             # a NaN minor axis gives lo = pmax / A
        (8.0, 0.0, 16, 1.0, 8),            # pmin 0: never below one texel
        (inf, 3.0, 16, inf, 1),            # lo = inf, q = inf / inf = NaN: one sample on the top level
        (4.0, 0.5, 16, 1.0, 4),            # pmin < 1 < pmax
        (40.0, 1.0, 16, 2.5, 16),          # a ratio above A: the minor axis is widened, N clamps
        (6.0, 4.0, 16, 4.0, 2),            # q = 1.5 rounds up
        (3.0, 3.0, 16, 3.0, 1),            # isotropic: q == 1
        (10.0, 3.0, 5, 3.0, 4),            # A no power of two, below the clamp
        (10.0, 1.5, 5, 2.0, 5),            # and at it
        (7.0, 2.0, 1, 7.0, 1),             # A = 1: lo = pmax
        (1.0000001, 0.0, 16, 1.0, 2),      # just minified: q barely above 1
    ]
    for pmax, pmin, A, want_rho, want_N in table:
        rho, N = aniso_ref.footprint(d([pmax]), d([pmin]), A)
        assert rho.dtype == np.float32 and N.dtype == np.int32
        assert_bit_equal(np.where(np.isnan(rho), d(0), rho), np.where(np.isnan(d([want_rho])), d(0), d([want_rho])),
                         f"rho of {(pmax, pmin, A)}")
        assert np.isnan(rho[0]) == np.isnan(want_rho)
        assert N[0] == want_N, (pmax, pmin, A, int(N[0]))
    # vectorised: the table at once, per A
    for A in {r[2] for r in table}:
        rows = [r for r in table if r[2] == A]
        rho, N = aniso_ref.footprint(d([r[0] for r in rows]), d([r[1] for r in rows]), A)
        assert N.tolist() == [r[4] for r in rows]


def test_axes_pick_the_longer_step_and_its_differences():
    d = np.float32
    u, v = d([0.5, 0.5, 0.5]), d([0.5, 0.5, 0.5])
    ux, vx = d([0.5 + 3 / 64, 0.5 + 1 / 64, np.nan]), d([0.5, 0.5, 0.5])
    uy, vy = d([0.5, 0.5, 0.5]), d([0.5 + 1 / 32, 0.5 + 4 / 32, 0.5 + 2 / 32])
    pmax, pmin, du, dv = aniso_ref.axes(u, v, ux, vx, uy, vy, 32, 64)
    assert pmax.tolist() == [3.0, 4.0, 2.0] and pmin.tolist()[:2] == [1.0, 1.0] and np.isnan(pmin[2])
    assert du.tolist() == [3 / 64, 0.0, 0.0] and dv.tolist() == [0.0, 4 / 32, 2 / 32]      # a NaN rx: y is the major axis


# ---- the four consequences ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("perspective", [False, True])
@pytest.mark.parametrize("name", ["trex256", "floor64"])
def test_the_four_consequences(scenes_, name, perspective):
    f, tri, uv, tex, chain = scenes_[name]
    th, tw = tex.shape[:2]
    base = f.color_buffer
    tri_pass = mip_ref.texture_pass(base, f.winner, tri, f.proj_mat, uv, tex, perspective=perspective, chain=chain)
    ys, xs, _, _, _, tl0, _ = mip_ref.pixel_levels(f.winner, tri, f.proj_mat, uv, th, tw, perspective)
    # 1. with A = 1 every pixel is the trilinear pixel
    one = aniso_ref.texture_pass(base, f.winner, tri, f.proj_mat, uv, tex, perspective, 1, chain=chain)
    assert_bit_equal(one, tri_pass, f"{name}: A = 1")
    for A in (2, 3, 5, 16):
        ys2, xs2, _, _, _, _, N, l0, _ = aniso_ref.pixel_footprints(f.winner, tri, f.proj_mat, uv, th, tw, perspective, A)
        assert np.array_equal(ys, ys2) and np.array_equal(xs, xs2)
        got = aniso_ref.texture_pass(base, f.winner, tri, f.proj_mat, uv, tex, perspective, A, chain=chain)
        assert not np.isnan(got).any()
        assert N.min() >= 1 and N.max() <= A
        # 2. every pixel with N == 1 is the trilinear pixel
        lone = N == 1
        assert_bit_equal(got[ys[lone], xs[lone]], tri_pass[ys[lone], xs[lone]], f"{name}: N = 1 at A = {A}")
        assert_bit_equal(got[f.winner < 0], base[f.winner < 0], "background")
        # 3. and 4.: the level is trilinear's or finer, by ceil(log2 A) at the most
        assert (l0 <= tl0).all() and (l0 >= tl0 - int(np.ceil(np.log2(A)))).all()
        assert (l0 < tl0).any() and (got != tri_pass).any(), (name, A, "anisotropy changed nothing")
        counts = np.bincount(N, minlength=17)
        print(f"{name}, perspective={perspective}, A={A}: N histogram {counts[1:].tolist()}")
        if A == 16:
            # conditions: the scenes reach what the tests are for
            if name == "trex256":
                assert len(ys) == 15801 and counts[1] == 0             # every covered pixel has N >= 2
            if name == "floor64":
                assert len(ys) == 1968
                if perspective:
                    assert (counts[1:] > 0).all() and counts[16] >= 100 and counts[1] >= 500
