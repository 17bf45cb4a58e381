"""The ambient-occlusion pass without a GPU: the header against the binding and the build lists, the entry point's
argument checks, the host model the GPU tests compare with (tests/ao_ref.py) on hand-built frames whose answer is known,
pinned on the oracle's frame of T-Rex by counts, by identities and against a float64 evaluation, the tap tables of
``ambient_occlusion.taps`` and ``Renderer``'s construction errors."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ao_ref
from pass_scenes import Frame, capi, trex_fixture  # noqa: F401 (fixtures)
from util import INCLUDE, assert_bit_equal, other_symbols, unit_in_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = [(1, 0), (-2, 2), (0, -3), (2, 3), (-4, -1), (4, -3), (-1, 5), (-3, -5), (5, 2), (-6, 2), (3, -6), (2, 6), (-6, -4),
         (7, -2), (-4, 6), (-1, -8)]
TREX_KW = dict(radius=0.03, radius_px=8, min_cos=0.1, strength=1.0, floor=0.0)


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_ao_header_symbol_is_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_ao.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["ao"]) == {"crender_ao_shade"}
    assert not declared & other_symbols(capi, "ao")
    L = capi.load()
    assert L.crender_ao_shade.argtypes == capi.UNIT_SIGNATURES["ao"]["crender_ao_shade"][1]
    # argument counts: the declaration's commas against the table
    decl = re.search(r"CRENDER_API int crender_ao_shade\((.*?)\);", header, re.S).group(1)
    res, args = capi.UNIT_SIGNATURES["ao"]["crender_ao_shade"]
    assert res == C.c_int and len(args) == len(decl.split(",")) == 21
    # the four floats of the declaration are the table's: radius, min_cos, strength and floor by value
    kinds = ["float" if re.match(r"\s*float \w+$", a) else "other" for a in decl.split(",")]
    assert [i for i, k in enumerate(kinds) if k == "float"] == [i for i, a in enumerate(args) if a is C.c_float] == [10, 11, 12, 13]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    limits = dict(re.findall(r"#define (CRENDER_AO_\w+) (\d+)", header))
    assert int(limits["CRENDER_AO_MAX_TAPS"]) == capi.AO_MAX_TAPS == ao_ref.MAX_TAPS == 64
    assert int(limits["CRENDER_AO_MAX_RADIUS_PX"]) == capi.AO_MAX_RADIUS_PX == ao_ref.MAX_RADIUS_PX == 32
    assert int(limits["CRENDER_AO_ROTATE"]) == capi.AO_ROTATE == 1
    assert int(limits["CRENDER_AO_FACE_NORMALS"]) == capi.AO_FACE_NORMALS == 2
    assert capi.ABI_VERSION == 6 and L.crender_abi_version() == 6


def test_ao_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit_in_build(_build, "ao", ["ao.hip"], [os.path.join(INCLUDE, "crender_ao.h")])
    # the kernel takes the shared pieces by inclusion, stages in LDS behind barriers and has no inline assembly
    unit = open(os.path.join(_build.SRC_DIR, "ao.hip")).read()
    for name in ("make_proj(", "wave_any(", "gather_corners("):
        assert name in unit and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name
    assert "extern __shared__" in unit and unit.count("__syncthreads()") == 2
    assert "asm" not in re.sub(r"//[^\n]*", "", unit)


def _projection(capi, H=8, W=8):
    P = (C.c_float * 16)()
    assert capi.load().crender_projection_matrix(45.0, 0.1, 1000.0, H, W, P) == capi.OK
    return P


def test_ao_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    good = _projection(capi)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    nan, inf = float("nan"), float("inf")

    def table(*pairs):
        return (C.c_int8 * (2 * len(pairs)))(*[v for p in pairs for v in p])
    one = table((1, 0))

    def shade(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=good, nrm=fake, taps=one, n=1, R=8, radius=0.03, min_cos=0.1,
              strength=2.0, floor=0.0, col=fake, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_ao_shade(win, z, tri, T, pos_of, P, nrm, taps, n, R, radius, min_cos, strength, floor, col,
                                  H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(z=None), dict(P=None), dict(taps=None), dict(col=None)):
        assert shade(**kw) == E and "is NULL" in text(), kw
    assert shade(nrm=None) == E and "d_normal is NULL without" in text()
    assert shade(nrm=None, flags=3, T=0) == capi.OK                 # the face mode reads no normal plane
    assert shade(tri=None, flags=2) == E and "d_tri is NULL" in text()
    assert shade(tri=None, T=0, flags=2) == capi.OK and shade(tri=None, T=0) == capi.OK
    assert shade(T=-1) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2)):
        assert shade(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert shade(**kw) == E and "rows outside the frame" in text(), kw
    many = table(*[(1 + i % 8, i // 8) for i in range(64)])
    for n in (0, 65, -1):
        assert shade(taps=many, n=n) == E and "n_taps is not 1 .. 64" in text(), n
    assert shade(taps=many, n=64, T=0) == capi.OK
    for R in (0, 33, -1):
        assert shade(R=R) == E and "radius_px is not 1 .. 32" in text(), R
    for pair in ((9, 0), (0, -9), (-9, 9), (127, 0), (-128, -128)):
        assert shade(taps=table((1, 1), pair), n=2) == E and "beyond radius_px" in text(), pair
    assert shade(taps=table((8, -8), (-8, 8)), n=2, T=0) == capi.OK
    assert shade(taps=table((1, 0), (0, 0)), n=2) == E and "(0, 0)" in text()
    assert shade(taps=table((1, 0), (0, 0)), n=1, T=0) == capi.OK    # a tap beyond n_taps is not looked at
    for bad in (nan, inf, -inf, 0.0, -0.03):
        assert shade(radius=bad) == E and "radius is not finite and positive" in text(), bad
    for bad in (nan, inf, -inf):
        for name in ("min_cos", "strength", "floor"):
            assert shade(**{name: bad}) == E and "not finite" in text(), (name, bad)
    assert shade(strength=-0.5) == E and "strength is negative" in text()
    for bad in (-0.01, 1.01):
        assert shade(floor=bad) == E and "floor is not 0 .. 1" in text(), bad
    assert shade(floor=1.0, strength=0.0, min_cos=-1.0, T=0) == capi.OK
    for i in (1, 2, 4, 6, 8, 9, 12, 13):
        P = _projection(capi)
        P[i] = 0.5
        assert shade(P=P) == E and "must be 0" in text(), i
        P[i] = nan
        assert shade(P=P) == E and "must be 0" in text(), i
    for i in (0, 5, 14):
        for bad in (0.0, nan, inf):
            P = _projection(capi)
            P[i] = bad
            assert shade(P=P) == E and "entry 0, 5 or 14" in text(), (i, bad)
    for flags in (4, 8, 0x80000000, 7):
        assert shade(flags=flags) == E and "unknown flag bits" in text(), flags
    assert text().startswith("crender_ao_shade")
    for flags in (0, 1, 2, 3):
        assert shade(T=0, flags=flags) == capi.OK


# ---- hand-built frames whose answer is known -------------------------------------------------------------------

def _plane_frame(oracle, H, W, depth_of_column):
    """A frame of planes facing the camera: column x lies at view depth depth_of_column(x); normals (0, 0, -1)."""
    P = oracle.projection_matrix(45.0, 0.1, 1000.0, H, W)
    zv = np.broadcast_to(np.float32(depth_of_column(np.arange(W))), (H, W)).astype(np.float32)
    z = (np.float32(P[2, 2]) + np.float32(P[3, 2]) / zv).astype(np.float32)
    winner = np.zeros((H, W), np.int32)
    normals = np.zeros((H, W, 3), np.float32)
    normals[..., 2] = -1.0
    color = np.full((H, W, 3), 200.0, np.float32)
    tri = np.zeros((1, 3, 3), np.float32)
    return color, z, winner, tri, P, normals


@pytest.mark.parametrize("rotate", [True, False])
def test_a_plane_facing_the_camera_is_not_occluded(oracle, rotate):
    frame = _plane_frame(oracle, 96, 96, lambda x: np.full(x.shape, 1.0))
    counts = {}
    out = ao_ref.ao_pass(*frame, TABLE, radius=0.05, radius_px=8, rotate=rotate, counts=counts)
    assert counts["covered"] == 96 * 96 and counts["occluded"] == 0 and counts["taps_taken"] == 0
    assert (counts["S"].view(np.uint32) == 0).all()                  # exactly +0
    assert_bit_equal(out, frame[0], "nothing is written")


@pytest.mark.parametrize("rotate", [True, False])
def test_a_depth_step_darkens_the_far_side_only(oracle, rotate):
    # 96 pixels across at 45 degrees: a pixel is 1 / (48 * 2.414) = 0.0086 wide at depth 1.  The step is 0.02 deep, so
    # under radius 0.05 a far pixel sees the near plane up to sqrt(0.05^2 - 0.02^2) = 0.046 = 5 pixels sideways.
    step = 50
    frame = _plane_frame(oracle, 96, 96, lambda x: np.where(x < step, 1.0, 1.02))
    counts = {}
    out = ao_ref.ao_pass(*frame, TABLE, radius=0.05, radius_px=8, rotate=rotate, counts=counts)
    changed = (out != frame[0]).any(2)
    assert changed.any() and counts["occluded"] == int(changed.sum())
    assert (out[changed] < 200.0).all()
    assert not changed[:, :step].any()                               # none of the near plane
    assert not changed[:, step + 8:].any()                           # and no further than radius_px from the step
    cols = np.nonzero(changed.any(0))[0]
    assert cols.min() == step and cols.max() < step + 8
    # a world radius smaller than the step's depth reaches nothing
    counts = {}
    out = ao_ref.ao_pass(*frame, TABLE, radius=0.015, radius_px=8, rotate=rotate, counts=counts)
    assert counts["occluded"] == 0 and counts["taps_taken"] == 0
    assert_bit_equal(out, frame[0], "radius below the step's depth")


# ---- the model on the oracle's frame of T-Rex ------------------------------------------------------------------

class _Frame(Frame):
    def run(self, taps=TABLE, **kw):
        for k, v in TREX_KW.items():
            kw.setdefault(k, v)
        return ao_ref.ao_pass(self.cam.color_buffer, self.cam.z_buffer, self.cam.winner, self.tri, self.cam.proj_mat,
                              self.cam.normals_buffer, taps, **kw)


trex = trex_fixture(_Frame)


@pytest.mark.parametrize("rotate,occluded,taken", [(True, 7102, 22461), (False, 7245, 22514)])
def test_the_counts_on_trex(trex, rotate, occluded, taken):
    counts = {}
    out = trex.run(rotate=rotate, counts=counts)
    assert not np.isnan(out).any()
    assert (counts["covered"], counts["occluded"], counts["taps_taken"]) == (15801, occluded, taken)
    assert round(counts["min_factor"], 4) == 0.7646
    # what the scene is chosen for: both sides are there
    assert occluded >= 0.05 * 15801 and 15801 - occluded >= 0.05 * 15801
    changed = (out.view(np.uint32) != trex.cam.color_buffer.view(np.uint32)).any(2)
    assert not changed[~trex.covered].any() and changed.sum() <= occluded
    assert (out <= trex.cam.color_buffer).all()


def test_the_table_is_what_taps_gives(trex):
    from cython3dmodelrenderer_amd import ambient_occlusion
    assert ambient_occlusion.taps(8, 16) == TABLE


def test_identities_bit_for_bit(trex):
    base = trex.cam.color_buffer
    # strength 0 under floor 1: every occluded pixel is multiplied by exactly 1
    a = trex.run(strength=0.0, floor=1.0)
    assert np.array_equal(a, base)
    # Sixteen taps that can never be taken — at 32 pixels, 0.1 of the view depth sideways, under a world radius of
    # 0.03 — add +0 to S sixteen times.  Their only trace is inv_n: 1/32 instead of 1/16, an exact halving, so with
    # twice the strength (an exact doubling) f is the same float: strength * (S * (1/16)) == 2 strength * (S * (1/32)).
    dead = [(32, k) for k in (-32, -9, 0, 17)] + [(-32, k) for k in (32, 5, -1, -20)] + \
           [(k, 32) for k in (-31, -8, 3, 19)] + [(k, -32) for k in (31, 7, -2, -18)]
    counts = {}
    trex.run(dead, radius_px=32, counts=counts)
    assert counts["taps_taken"] == 0 and counts["occluded"] == 0
    for rotate in (True, False):
        alone = trex.run(TABLE, radius_px=32, strength=0.75, rotate=rotate)
        both = trex.run(TABLE + dead, radius_px=32, strength=1.5, rotate=rotate)
        assert_bit_equal(both, alone, f"dead taps, rotate={rotate}")
        assert (alone != base).any()
    # radius_px bounds the table and sizes the halo: it is in no statement
    assert_bit_equal(trex.run(radius_px=32), trex.run(radius_px=8), "radius_px")


def test_without_rotate_every_pixel_uses_the_table_as_given(trex):
    turns = [lambda dx, dy: (dx, dy), lambda dx, dy: (-dy, dx), lambda dx, dy: (dy, -dx), lambda dx, dy: (-dx, -dy)]
    rot = {}
    trex.run(rotate=True, counts=rot)
    r_of = (rot["xs"] & 1) | ((rot["ys"] & 1) << 1)
    differ = 0
    for r, turn in enumerate(turns):
        plain = {}
        trex.run([turn(dx, dy) for dx, dy in TABLE], rotate=False, counts=plain)
        # the unrotated pass over the table turned by hand is, at the pixels of parity r, the rotating pass
        assert_bit_equal(plain["S"][r_of == r], rot["S"][r_of == r], f"parity {r}")
        assert (r_of == r).sum() > 3000
        differ += int((plain["S"][r_of != r] != rot["S"][r_of != r]).sum())
    assert differ > 1000                   # and elsewhere the turn matters: the comparison can fail


def test_against_the_statements_in_float64(trex):
    """The same statements from the same float32 planes in float64.  Measured on this frame: the largest absolute
    difference of a colour (values up to 255) is 3.93e-4 with the rotation and 3.11e-4 without — larger than the Phong
    pass's, since D is a difference of two nearby view points and c divides by its length.  The assertion is four times
    the larger, rounded up to a power of two, 2^-9 = 1.95e-3.  It is a check of the model's statements, not a bound on
    the kernel, which is held to bit equality with the float32 model.  Pixels whose float32 and float64 evaluations
    take a different set of taps (a comparison within an ulp of its threshold) would differ by whole taps: there is
    none on this frame."""
    for rotate in (True, False):
        a = trex.run(rotate=rotate)
        b = trex.run(rotate=rotate, dtype=np.float64)
        assert a.dtype == np.float32 and b.dtype == np.float64
        diff = float(np.abs(a.astype(np.float64) - b).max())
        print(f"largest |float32 - float64| colour difference, rotate={rotate}: {diff:.3e}")
        assert 0 < diff <= 2.0 ** -9


# ---- ambient_occlusion.taps and Renderer -----------------------------------------------------------------------

@pytest.mark.parametrize("radius_px,n", [(1, 8), (8, 16), (16, 32), (32, 64)])
def test_tap_tables(radius_px, n):
    from cython3dmodelrenderer_amd import ambient_occlusion
    t = ambient_occlusion.taps(radius_px, n)
    assert len(t) == n and len(set(t)) == n and (0, 0) not in t
    assert all(isinstance(v, int) for p in t for v in p)
    assert all(abs(dx) <= radius_px and abs(dy) <= radius_px for dx, dy in t)
    assert t == ambient_occlusion.taps(radius_px, n)                 # deterministic
    a = np.array(t)
    # spread over the disc: every quadrant gets its share, and the taps reach the outer half of the radius
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        assert ((a[:, 0] * sx >= 0) & (a[:, 1] * sy >= 0)).sum() >= n // 8
    assert (np.hypot(a[:, 0], a[:, 1]) > radius_px / 2).sum() >= n // 2
    if radius_px > 1:
        assert (np.hypot(a[:, 0], a[:, 1]) <= radius_px + 0.5).all()   # the spiral stays inside the disc


def test_tap_tables_errors():
    from cython3dmodelrenderer_amd import ambient_occlusion
    assert sorted(ambient_occlusion.taps(1, 8)) == sorted((dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy) != (0, 0))
    with pytest.raises(ValueError, match="9 taps do not fit radius_px=1: the square holds 8"):
        ambient_occlusion.taps(1, 9)
    with pytest.raises(ValueError, match="25 taps do not fit radius_px=2"):
        ambient_occlusion.taps(2, 25)
    assert len(ambient_occlusion.taps(2, 24)) == 24
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="radius_px must be a positive int"):
            ambient_occlusion.taps(bad, 4)
        with pytest.raises(ValueError, match="number of taps must be a positive int"):
            ambient_occlusion.taps(4, bad)


def test_renderer_construction():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer

    class WithPass:
        def ao_pass(self):
            pass

    class Plain:
        pass
    light = GuroIllumination((0.3, -0.2, 1.0))
    with pytest.raises(ValueError, match="ambient-occlusion pass.*Plain has no ao_pass"):
        Renderer(Plain(), light, ambient_occlusion={})
    assert Renderer(Plain(), light).ambient_occlusion is None
    opts = dict(radius=0.05, taps=8)
    r = Renderer(WithPass(), light, ambient_occlusion=opts)
    assert r.ambient_occlusion == opts and r.ambient_occlusion is not opts
    assert Renderer(WithPass(), light, ambient_occlusion={}).ambient_occlusion == {}
    assert "ambient_occlusion" in inspect.signature(Renderer.__init__).parameters
