"""The environment pass without a GPU: the header against the binding and the build tables, the entry point's argument
checks, the host model the GPU tests compare with (tests/env_ref.py) pinned on the oracle's frames — by counts, by
identities and against a float64 evaluation —, the layout of the cube's chain, and the cube makers of
``cython3dmodelrenderer_amd.environment``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import env_ref
import mip_ref
from pass_scenes import Frame, Soup, capi, trex_fixture  # noqa: F401 (fixtures)
from util import assert_bit_equal, other_symbols, own_unit_source, random_soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "crender_env_shade"
_vp, _i32, _i64, _u32, _f, _fp = C.c_void_p, C.c_int, C.c_int64, C.c_uint, C.c_float, C.POINTER(C.c_float)
SIGNATURE = [_vp, _vp, _i64, _vp, _fp, _vp, _vp, _i32, _vp, _i32, _f, _fp, _f, _f, _fp, _f, _vp, _i32, _i32, _i32, _i32, _u32, _vp]


def _tilted():
    """The orientation whose z axis — where the camera looks — is (1, 1, 1) / sqrt 3 of the cube's frame."""
    z = np.ones(3) / np.sqrt(3.0)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1).astype(np.float32)


def _cube(seed=5, S=8):
    return np.random.default_rng(seed).integers(0, 256, (6, S, S, 3), dtype=np.uint8)


class _Frame(Frame):
    def run(self, levels, normals=None, winner=None, **kw):
        return env_ref.env_pass(self.cam.color_buffer, self.cam.winner if winner is None else winner, self.tri,
                                self.cam.proj_mat, self.cam.normals_buffer if normals is None else normals, levels, **kw)


trex = trex_fixture(_Frame)


@pytest.fixture(scope="module")
def soup(oracle):
    m = Soup()
    return _Frame(oracle, (m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles), 256, 256)


@pytest.fixture(scope="module")
def small_soups(oracle):
    """Soups 51 and 61 of tests/test_phong_gpu.py."""
    return {51: _Frame(oracle, random_soup(np.random.default_rng(51), 4000, 200, size_px=(1.0, 40.0)), 200, 173),
            61: _Frame(oracle, random_soup(np.random.default_rng(61), 300, 40, size_px=(3.0, 25.0)), 40, 37)}


# ---- 1. the host side of the ABI -------------------------------------------------------------------------------------

def test_env_symbol_is_declared_bound_and_exported(capi):
    header = open(os.path.join(ROOT, "include", "crender_env.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["env"]) == {ENTRY}
    assert not declared & other_symbols(capi, "env")
    res, args = capi.UNIT_SIGNATURES["env"][ENTRY]
    L = capi.load()
    assert res == C.c_int and args == SIGNATURE == getattr(L, ENTRY).argtypes
    decl = re.search(r"CRENDER_API int " + ENTRY + r"\((.*?)\);", header, re.S).group(1).split(",")
    assert len(decl) == len(args) == 23
    # the floats of the declaration are the table's: level_frac, reflectivity, f0, background_gain
    floats = [i for i, a in enumerate(decl) if re.match(r"\s*float \w+$", a)]
    assert floats == [i for i, a in enumerate(args) if a is _f] == [10, 12, 13, 15]
    names = [re.search(r"(\w+)$", a.strip()).group(1) for a in decl]
    assert names == ["d_winner", "d_tri", "T", "d_pos_of", "P16", "d_normal", "d_faces0", "S0", "d_faces1", "S1", "level_frac",
                     "M9", "reflectivity", "f0", "tint3", "background_gain", "d_color", "H", "W", "y0", "y1", "flags", "stream"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert ENTRY in set(re.findall(r" T (crender_\w+)", out))
    defines = dict(re.findall(r"#define (CRENDER_ENV_\w+) (\d+)u?", header))
    assert (int(defines["CRENDER_ENV_REFLECT"]), int(defines["CRENDER_ENV_BACKGROUND"])) == \
        (capi.ENV_REFLECT, capi.ENV_BACKGROUND) == (env_ref.REFLECT, env_ref.BACKGROUND) == (1, 2)
    assert int(defines["CRENDER_ENV_MAX_SIDE"]) == capi.ENV_MAX_SIDE == env_ref.MAX_SIDE == 8192
    assert capi.ABI_VERSION == 6


def test_env_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit = new = own_unit_source(_build, "env", "envmap.hip", "crender_env.h")
    head = "// ---- environment mapping (crender_env_shade) ----"
    assert unit.count(head) == 1 and unit.index(head) < unit.index("void k_env_shade") < unit.index("int crender_env_shade(")
    assert new.count("namespace {") == 1 and new.count('extern "C" {') == 1
    # the pass takes the passes' frame and the sample from the shared header, as they are
    for name in ("winner_pixel(", "winner_triangle(", "barycentric(", "bilinear(", "wave_any(", "pass_grid(", "frame_checks(",
                 "rows_check(", "make_proj("):
        assert name in new and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name
    assert "__shared__" not in new
    # six instances
    assert len(set(re.findall(r"k_env_shade<(?:true|false), (?:true|false), (?:true|false)>", new))) == 6


# ---- 2. argument errors ----------------------------------------------------------------------------------------------

def test_env_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first or launches nothing
    nan, inf = float("nan"), float("inf")
    P = capi.f32_16(np.diag(np.float32([2.4, 2.4, 1.0, 0.0])))
    eye = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    white = (C.c_float * 3)(1.0, 1.0, 1.0)
    R, B = capi.ENV_REFLECT, capi.ENV_BACKGROUND

    def shade(win=fake, tri=fake, T=4, pos_of=None, P=P, nrm=fake, f0_=fake, S0=8, f1_=None, S1=0, frac=0.0, M=eye, refl=1.0,
              f0=0.04, tint=white, gain=1.0, col=fake, H=8, W=8, y0=0, y1=8, flags=R):
        return L.crender_env_shade(win, tri, T, pos_of, P, nrm, f0_, S0, f1_, S1, frac, M, refl, f0, tint, gain, col, H, W, y0,
                                   y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    # 1. NULL pointers; the normal plane only with REFLECT
    for kw in (dict(win=None), dict(P=None), dict(f0_=None), dict(M=None), dict(tint=None), dict(col=None), dict(nrm=None)):
        assert shade(**kw) == E and "is NULL" in text(), kw
    # 2. the frame and the rows
    assert shade(tri=None) == E and "NULL with T > 0" in text()
    assert shade(T=-1) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2)):
        assert shade(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3)):
        assert shade(**kw) == E and "rows outside the frame" in text(), kw
    # 3. the sides
    for S0 in (0, -1, 8193):
        assert shade(S0=S0) == E and "S0 is not 1 .. 8192" in text(), S0
    for S1 in (-1, 8193):
        assert shade(S1=S1) == E and "S1 is not 0 .. 8192" in text(), S1
    # 4. the second level: all of it or none
    for kw in (dict(f1_=fake), dict(f1_=fake, S1=4), dict(f1_=fake, S1=4, frac=1.0), dict(f1_=fake, S1=4, frac=nan),
               dict(f1_=fake, S1=4, frac=-0.5), dict(S1=4), dict(frac=0.5), dict(S1=4, frac=0.5), dict(f1_=fake, frac=0.5)):
        assert shade(**kw) == E and "neither all given" in text(), kw
    # (the order: a bad row comes before a bad side, a bad side before the triple, the triple before the values)
    assert shade(y0=-1, S0=0) == E and "rows" in text()
    assert shade(S0=0, frac=0.5) == E and "S0" in text()
    assert shade(frac=0.5, refl=2.0) == E and "neither all given" in text()
    # 5. finiteness and ranges
    for bad in (nan, inf, -inf):
        for i in range(9):
            m = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
            m[i] = bad
            assert shade(M=(C.c_float * 9)(*m)) == E and "not finite" in text(), (bad, i)
        for i in range(3):
            t3 = [1.0] * 3
            t3[i] = bad
            assert shade(tint=(C.c_float * 3)(*t3)) == E and "not finite" in text(), (bad, i)
        assert shade(gain=bad) == E and "not finite" in text(), bad
    for kw in (dict(refl=-0.01), dict(refl=1.5), dict(refl=nan), dict(f0=-1.0), dict(f0=1.001), dict(f0=nan)):
        assert shade(**kw) == E and "reflectivity or f0 is not 0 .. 1" in text(), kw
    assert shade(gain=-1.0) == E and "background_gain is negative" in text()
    assert shade(refl=nan, flags=7) == E and "reflectivity" in text()            # before the flags
    # 6. the projection, with BACKGROUND only
    for i in (0, 5):
        for bad in (0.0, nan, inf):
            m = np.diag(np.float32([2.4, 2.4, 1.0, 0.0])).reshape(16)
            m[i] = bad
            Pb = (C.c_float * 16)(*m.tolist())
            assert shade(P=Pb, flags=R | B) == E and "entry 0 or 5" in text(), (i, bad)
            assert shade(P=Pb, T=0, tri=None) == capi.OK
    # 7. flags
    for flags in (4, 7, 0x80000001):
        assert shade(flags=flags) == E and "unknown flag bits" in text(), flags
    assert shade(flags=0) == E and "neither CRENDER_ENV_REFLECT nor CRENDER_ENV_BACKGROUND" in text()
    assert text().startswith("crender_env_shade: ")
    # nothing to launch: no triangles or no reflectivity, with REFLECT alone; the second level may be there
    assert shade(T=0, tri=None) == capi.OK and shade(T=0) == capi.OK
    assert shade(refl=0.0) == capi.OK and shade(refl=-0.0) == capi.OK
    assert shade(T=0, f1_=fake, S1=4, frac=0.5) == capi.OK and shade(T=0, S0=8192, f1_=fake, S1=1, frac=0.999) == capi.OK
    assert shade(T=0, nrm=None, flags=B, S0=0) == E            # without REFLECT the normal plane is not asked for


# ---- 3. the model's counts on the oracle's frames --------------------------------------------------------------------

TREX_FACES = [726, 4234, 4478, 2051, 1527, 2785]
SOUP_FACES = [12156, 10971, 9480, 10516, 13860, 8456]


def test_the_counts_on_trex_and_the_soup(trex, soup):
    for s, covered, faces in ((trex, 15801, TREX_FACES), (soup, 65439, SOUP_FACES)):
        counts = {}
        out = s.run(_cube(), counts=counts)
        assert not np.isnan(out).any()
        assert (counts["covered"], counts["written"], counts["faces"]) == (covered, covered, faces)
        assert sum(faces) == covered and min(faces) >= 0.02 * covered          # what the scenes are chosen for
        assert counts["background"] == 0 and (counts["face"] >= 0).sum() == covered
        bg = ~((s.cam.winner >= 0) & (s.cam.winner < len(s.tri)))
        assert_bit_equal(out[bg], s.cam.color_buffer[bg], "the background is not written")
        assert (out[~bg].view(np.uint32) != s.cam.color_buffer[~bg].view(np.uint32)).any(1).mean() > 0.99


# ---- 4. identities, bit for bit --------------------------------------------------------------------------------------

def test_a_flipped_normal_plane_and_no_reflectivity(trex):
    cube = _cube()
    a = trex.run(cube, orientation=_tilted(), tint=(1.0, 0.5, 0.25), f0=0.3)
    b = trex.run(cube, normals=-trex.cam.normals_buffer, orientation=_tilted(), tint=(1.0, 0.5, 0.25), f0=0.3)
    assert_bit_equal(a, b, "n -> -n")
    assert (a != trex.cam.color_buffer).any()
    assert_bit_equal(trex.run(cube, reflectivity=0.0), trex.cam.color_buffer, "reflectivity = 0")
    assert_bit_equal(trex.run(cube, reflect=False), trex.cam.color_buffer, "without REFLECT")


def test_a_mirror_of_one_colour(trex):
    """f0 = 1 and reflectivity = 1 give w = 1 * (1 + 0 * m5) = 1, so a pixel becomes c * 0 + e.  The Bilinear statement
    returns E itself from four texels E when the products E * weight are exact — E a power of two — since
    fl(fl(1 - a) + a) = 1 for every weight a in [0, 1): so E is made of powers of two."""
    E = np.float32([128.0, 64.0, 2.0])
    cube = np.broadcast_to(E.astype(np.uint8), (6, 4, 4, 3)).copy()
    for kw in (dict(), dict(level=1.5), dict(orientation=_tilted())):
        out = trex.run(env_ref.chain_levels(cube), f0=1.0, reflectivity=1.0, **kw)
        assert_bit_equal(out[trex.covered], np.broadcast_to(E, (15801, 3)), f"a mirror, {kw}")
        assert_bit_equal(out[~trex.covered], trex.cam.color_buffer[~trex.covered], "the background")


def _turned_cube(cube, M):
    """(the cube that shows under the identity what `cube` shows under the signed permutation M; the faces of it whose sc
    and tc are the ones `cube`'s face has under M: on them the two lookups run the same float32 statements).  The face
    map comes from ``face_direction``: the direction of every texel's centre, carried by M, names the texel it shows."""
    from cython3dmodelrenderer_amd.environment import face_direction
    S = cube.shape[1]
    c = (2.0 * np.arange(S) + 1.0) / S - 1.0
    t, s = np.meshgrid(c, c, indexing="ij")
    out = np.empty_like(cube)
    same = []
    for k in range(6):
        v = np.stack(face_direction(k, s, t), -1) @ np.asarray(M, np.float64).T
        face, sc, tc, ma = env_ref.face_of([v[..., 0], v[..., 1], v[..., 2]])
        assert (ma == 1).all() and len(np.unique(face)) == 1
        col, row = ((sc + 1.0) * S - 1.0) / 2.0, ((tc + 1.0) * S - 1.0) / 2.0
        assert (col == np.rint(col)).all() and (row == np.rint(row)).all()
        out[k] = cube[face, row.astype(int), col.astype(int)]
        if (sc == s).all() and (tc == t).all():
            same.append(k)
    return out, same


@pytest.mark.parametrize("name,M,same", [
    ("half a turn about y", np.diag([-1.0, 1.0, -1.0]), [0, 1, 4, 5]),
    ("x -> y -> z -> x", [[0, 0, 1], [1, 0, 0], [0, 1, 0]], None),
    ("a mirror and a quarter turn", [[0, -1, 0], [-1, 0, 0], [0, 0, 1]], None),
])
def test_a_signed_permutation_is_a_turned_cube(trex, name, M, same):
    """d = M r is exact for a signed permutation, so the lookup under M reads the texels the identity reads in the turned
    cube.  Where the turned face keeps sc and tc the two run the same statements: bit for bit.  Elsewhere sc and tc change
    places or signs, and the Bilinear statement is not symmetric under either in float32 (1 + q and 1 - q round
    differently; the blend runs along x first): there the two agree to the rounding of the texel coordinates.  A
    coordinate f = tu * S - 0.5 is at most S and comes from four operations of relative error 2^-24 each, so either
    evaluation is within 4 S 2^-24 of the exact one and the two within S 2^-21 of each other; a bilinear sample moves by
    at most 255 per texel along either axis, so the samples differ by at most 2 * 255 * S * 2^-21 = 1.95e-3 at S = 8, and
    the blends' own roundings (seven operations on values up to 255: 7 * 255 * 2^-24 = 1.1e-4 each) add 2.2e-4.  The
    weight w <= 1 and the unit tint scale that by at most 1: the bound is 2^-8 = 3.9e-3."""
    cube = _cube()
    turned, keeps = _turned_cube(cube, M)
    assert same is None or keeps == same
    ca, cb = {}, {}
    a = trex.run(cube, orientation=np.float32(M), f0=0.5, counts=ca)
    b = trex.run(turned, f0=0.5, counts=cb)
    assert ca["written"] == cb["written"] == 15801
    exact = np.isin(cb["face"], keeps)
    assert exact.sum() == sum(cb["faces"][k] for k in keeps)
    assert_bit_equal(a[exact], b[exact], f"{name}: the faces that keep sc and tc")
    assert_bit_equal(a[~trex.covered], b[~trex.covered], f"{name}: the background")
    diff = float(np.abs(a - b).max())
    print(f"{name}: {int(exact.sum())} pixels bit for bit, the others within {diff:.3e}")
    assert diff <= 2.0 ** -8
    assert diff > 0                               # (some face is turned: the two are not the same statements)
    # and the background reads the turned cube alike
    a = trex.run(cube, orientation=np.float32(M), reflect=False, background=1.0, counts=ca)
    b = trex.run(turned, reflect=False, background=1.0, counts=cb)
    assert sum(cb["background_faces"]) == 49735 == cb["background_faces"][4]
    if 4 in keeps:
        assert_bit_equal(a, b, f"{name}: the background, bit for bit")
    assert float(np.abs(a - b).max()) <= 2.0 ** -8


def test_a_whole_level_is_that_level_bound_alone(trex):
    levels = env_ref.chain_levels(_cube())
    assert [l.shape[1] for l in levels] == [8, 4, 2, 1]
    assert_bit_equal(trex.run(levels, level=1.0), trex.run(levels[1]), "level 1.0")
    assert_bit_equal(trex.run(levels, level=3.0), trex.run(levels[3]), "the last level")
    assert_bit_equal(trex.run(levels, level=3), trex.run(levels, level=2.9999999999), "a fraction that rounds up")
    half = trex.run(levels, level=0.5)
    assert (half != trex.run(levels)).any() and (half != trex.run(levels[1])).any()
    # between two levels the sample is between theirs (up to the blend's rounding); w and the tint only scale it
    lo, hi = trex.run(levels, f0=1.0), trex.run(levels[1], f0=1.0)
    mid = trex.run(levels, level=0.25, f0=1.0)
    assert (mid >= np.minimum(lo, hi) - 1e-4).all() and (mid <= np.maximum(lo, hi) + 1e-4).all()


def test_the_chain_of_the_stacked_faces_is_six_chains(trex):
    """What ``bind_environment(mipmaps=True)`` relies on: the levels 0 .. log2 S of the texture chain of the [6 S, S, 3]
    image are, face by face, the chains of the six faces, level j of face k at offset_j + k * 3 * S_j ** 2."""
    cube = _cube(seed=6, S=16)
    levels, offsets, total = mip_ref.layout(96, 16)
    assert levels[:5] == [(96, 16), (48, 8), (24, 4), (12, 2), (6, 1)]
    packed = mip_ref.pack_chain(mip_ref.build_chain(cube.reshape(96, 16, 3)))
    assert len(packed) == total
    own = env_ref.chain_levels(cube)
    for k in range(6):
        alone = mip_ref.build_chain(cube[k])
        for j in range(5):
            side = 16 >> j
            at = offsets[j] + k * 3 * side * side
            assert np.array_equal(packed[at:at + 3 * side * side].reshape(side, side, 3), alone[j]), (k, j)
            assert np.array_equal(own[j][k], alone[j]), (k, j)


# ---- 5. the background -----------------------------------------------------------------------------------------------

def test_the_background(trex):
    cube = _cube()
    counts = {}
    out = trex.run(cube, reflect=False, background=0.5, counts=counts)
    assert counts["background"] == 49735 and counts["background_faces"] == [0, 0, 0, 0, 49735, 0]    # fov 45: all +z
    assert_bit_equal(out[trex.covered], trex.cam.color_buffer[trex.covered], "covered pixels are not written")
    assert (out[~trex.covered] <= 127.5).all() and out[~trex.covered].max() > 100
    both = trex.run(cube, background=0.5)
    assert_bit_equal(both[~trex.covered], out[~trex.covered], "both flags: the background")
    assert_bit_equal(both[trex.covered], trex.run(cube)[trex.covered], "both flags: the reflection")
    # winners that name no triangle are background
    odd = trex.cam.winner.copy()
    odd[:8] = len(trex.tri)
    odd[8:16] = -7
    trex.run(cube, winner=odd, reflect=False, background=1.0, counts=counts)
    assert counts["background"] == int(((odd < 0) | (odd >= len(trex.tri))).sum()) == sum(counts["background_faces"])
    # looking along (1, 1, 1): three faces share the frame, and T-Rex's background
    trex.run(cube, winner=np.full_like(odd, -1), orientation=_tilted(), reflect=False, background=1.0, counts=counts)
    share = [v / 65536.0 for v in counts["background_faces"]]
    print("the shares of a full frame along (1, 1, 1):", [f"{100 * v:.1f} %" for v in share])
    assert counts["background"] == 65536 and min(share[0], share[2], share[4]) >= 0.10 and share[1] == share[3] == share[5] == 0
    trex.run(cube, orientation=_tilted(), reflect=False, background=1.0, counts=counts)
    assert sum(counts["background_faces"]) == 49735
    assert min(counts["background_faces"][k] for k in (0, 2, 4)) >= 0.05 * 49735


# ---- 6. against itself in float64 ------------------------------------------------------------------------------------

# The largest |float32 - float64| of a written colour (values up to 255), pixels whose face differs left out, as measured
# with this model on T-Rex 256^2, the default soup and the soups 51 and 61 of tests/test_phong_gpu.py: under the random 8^3 cube, where a texel
# step is up to 255 and the error of a texel coordinate counts, and under the smooth sky.
MEASURED_RANDOM, MEASURED_SKY = 1.361e-4, 8.573e-5


def test_against_the_statements_in_float64(trex, soup, small_soups):
    """The same statements from the same float32 barycentrics in float64.  The face is a comparison of rounded
    magnitudes: at most 0.1 % of the written pixels may pick another face in float64 (none does on these four frames).
    The colours are held to ten times the measured difference, the project's margin for these self-checks.  A check of
    the model's statements, not a bound on the kernel, which is held to bit equality with the float32 model."""
    from cython3dmodelrenderer_amd.environment import gradient_sky
    frames = dict(trex=trex, soup=soup, soup51=small_soups[51], soup61=small_soups[61])
    for what, levels, measured in (("random", _cube(), MEASURED_RANDOM), ("sky", gradient_sky(8), MEASURED_SKY)):
        worst = 0.0
        for name, s in frames.items():
            ca, cb = {}, {}
            a = s.run(levels, counts=ca)
            b = s.run(levels, counts=cb, dtype=np.float64)
            assert a.dtype == np.float32 and b.dtype == np.float64
            written = (ca["face"] >= 0) | (cb["face"] >= 0)
            other = ca["face"] != cb["face"]
            assert other.sum() <= 0.001 * written.sum(), (what, name, int(other.sum()))
            diff = float(np.abs(a.astype(np.float64) - b)[written & ~other].max())
            print(f"{what} cube, {name}: {int(other.sum())} of {int(written.sum())} faces differ, largest |float32 - float64| {diff:.3e}")
            worst = max(worst, diff)
        assert 0 < worst <= 10 * measured, (what, worst)


# ---- 7. the cube makers ----------------------------------------------------------------------------------------------

def test_face_direction_inverts_the_table():
    from cython3dmodelrenderer_amd.environment import face_direction
    rng = np.random.default_rng(7)
    s, t = rng.uniform(-0.999, 0.999, (2, 500))
    for k in range(6):
        face, sc, tc, ma = env_ref.face_of(list(face_direction(k, s, t)))
        assert (face == k).all() and (ma == 1).all() and np.array_equal(sc, s) and np.array_equal(tc, t)
    for bad in (-1, 6):
        with pytest.raises(ValueError, match="face must be 0 .. 5"):
            face_direction(bad, 0.0, 0.0)


def test_cube_from_equirect_of_a_panorama_that_is_constant_per_face():
    from cython3dmodelrenderer_amd.environment import cube_from_equirect
    colours = np.uint8([[250, 10, 10], [10, 250, 10], [10, 10, 250], [250, 250, 10], [10, 250, 250], [250, 10, 250]])
    Hp, Wp = 256, 512
    lat = (0.5 - (np.arange(Hp) + 0.5) / Hp) * np.pi
    lon = ((np.arange(Wp) + 0.5) / Wp - 0.5) * 2.0 * np.pi
    d = [np.cos(lat)[:, None] * np.sin(lon)[None, :], -np.sin(lat)[:, None] * np.ones(Wp)[None, :],
         np.cos(lat)[:, None] * np.cos(lon)[None, :]]
    pano = colours[env_ref.face_of(d)[0]]
    cube = cube_from_equirect(pano, 4)            # (its texel centres lie a quarter of a face from the seams)
    assert cube.shape == (6, 4, 4, 3) and cube.dtype == np.uint8
    assert np.array_equal(cube, np.broadcast_to(colours[:, None, None, :], (6, 4, 4, 3)))
    with pytest.raises(ValueError, match="uint8"):
        cube_from_equirect(pano.astype(np.float32), 4)
    with pytest.raises(ValueError, match="S must be"):
        cube_from_equirect(pano, 0)


def test_gradient_sky_is_the_right_way_up(oracle):
    from cython3dmodelrenderer_amd.environment import gradient_sky
    zenith, horizon, ground = (10, 20, 250), (200, 200, 200), (90, 60, 30)
    sky = gradient_sky(16, zenith, horizon, ground)
    assert sky.shape == (6, 16, 16, 3) and sky.dtype == np.uint8
    # y grows with the row: +y is down, the ground; -y is up, the zenith; their middles are nearest the poles
    assert np.abs(sky[2, 7:9, 7:9].astype(int) - ground).max() <= 3 and np.abs(sky[3, 7:9, 7:9].astype(int) - zenith).max() <= 3
    for k in (0, 1, 4, 5):            # the side faces: blue falls and red rises from the top row to the horizon, row 0 is up
        assert (np.diff(sky[k, :8, :, 2].astype(int), axis=0) <= 0).all() and sky[k, 0, 8, 2] > sky[k, 7, 8, 2] > sky[k, 15, 8, 2]
        assert np.abs(sky[k, 7:9].astype(int) - horizon).max() <= 12
    # painted behind an empty frame by the model: the upper rows are nearer the zenith, the lower ones the ground
    cam = oracle.OracleFiller(64, 64, fov=45.0)
    empty = np.full((64, 64), -1, np.int32)
    tri = np.zeros((0, 3, 3), np.float32)
    out = env_ref.env_pass(np.zeros((64, 64, 3), np.float32), empty, tri, cam.proj_mat, np.zeros((64, 64, 3), np.float32),
                           gradient_sky(64, zenith, horizon, ground), reflect=False, background=1.0)
    assert out[0, :, 2].min() > out[31, :, 2].max() > out[63, :, 2].max()          # blue falls down the frame
    assert out[0, :, 0].max() < out[31, :, 0].min() and out[63, :, 0].max() < out[32, :, 0].min()   # red peaks at the horizon
    # looking up, the frame's middle is the zenith
    up = np.float32([[1, 0, 0], [0, 0, -1], [0, 1, 0]])
    out = env_ref.env_pass(np.zeros((64, 64, 3), np.float32), empty, tri, cam.proj_mat, np.zeros((64, 64, 3), np.float32),
                           gradient_sky(64, zenith, horizon, ground), reflect=False, background=1.0, orientation=up)
    assert np.abs(out[31:33, 31:33] - np.float32(zenith)).max() <= 2.0


# ---- 8. the Renderer's option, as far as it needs no GPU -------------------------------------------------------------

def test_renderer_option_errors_without_a_gpu():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer

    class Plain:
        pass

    class WithPass:
        bound = None

        def environment_pass(self, **kw):
            pass

        def bind_environment(self, faces, mipmaps=False):
            self.bound = (faces, mipmaps)

    cube = _cube()
    with pytest.raises(ValueError, match="no environment_pass"):
        Renderer(Plain(), GuroIllumination((0.3, -0.2, 1.0)), environment=dict(faces=cube))
    with pytest.raises(ValueError, match=r"\['roughness'\] unknown"):
        Renderer(WithPass(), GuroIllumination((0.3, -0.2, 1.0)), environment=dict(faces=cube, roughness=0.5))
    with pytest.raises(ValueError, match="needs 'faces'"):
        Renderer(WithPass(), GuroIllumination((0.3, -0.2, 1.0)), environment=dict(level=1.0))
    f = WithPass()
    r = Renderer(f, GuroIllumination((0.3, -0.2, 1.0)), environment=dict(faces=cube, level=1.5, background=True))
    assert f.bound[0] is cube and f.bound[1] is True and r.environment == dict(level=1.5, background=True)
    f = WithPass()
    r = Renderer(f, GuroIllumination((0.3, -0.2, 1.0)), environment=dict(faces=cube, f0=1.0))
    assert f.bound[1] is False and r.environment == dict(f0=1.0)
    assert Renderer(f, GuroIllumination((0.3, -0.2, 1.0))).environment is None
