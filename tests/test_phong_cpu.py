"""The Phong pass without a GPU: the header against the binding and the build lists, the entry point's argument
checks, the host model the GPU tests compare with (tests/phong_ref.py) pinned on the oracle's frame of T-Rex — against
``oracle.guro`` in the directional, diffuse-only case, by counts, by identities and against a float64 evaluation —
and the ``PhongIllumination`` class."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import phong_ref
from pass_scenes import Frame, capi, trex_fixture  # noqa: F401 (fixtures)
from util import INCLUDE, assert_bit_equal, other_symbols, unit_in_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GURO = (0.3, -0.2, 1.0)              # what GuroIllumination is constructed with
POINT = (-0.8, -0.5, -0.2)           # a point light up and to the left of the camera, a little behind it
SECOND = (1.5, -2.0, -0.5)           # and one far to the right: a third of the model faces away from it


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_phong_header_symbol_is_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_phong.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["phong"]) == {"crender_phong_shade"}
    assert not declared & other_symbols(capi, "phong")
    L = capi.load()
    assert L.crender_phong_shade.argtypes == capi.UNIT_SIGNATURES["phong"]["crender_phong_shade"][1]
    # argument counts: the declaration's commas against the table
    decl = re.search(r"CRENDER_API int crender_phong_shade\((.*?)\);", header, re.S).group(1)
    res, args = capi.UNIT_SIGNATURES["phong"]["crender_phong_shade"]
    assert res == C.c_int and len(args) == len(decl.split(",")) == 20
    # the two floats of the declaration are the table's: ambient and clamp by value, the host arrays as pointers
    kinds = ["float" if re.match(r"\s*float \w+$", a) else "other" for a in decl.split(",")]
    assert [i for i, k in enumerate(kinds) if k == "float"] == [i for i, a in enumerate(args) if a is C.c_float] == [9, 12]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    limits = dict(re.findall(r"#define (CRENDER_PHONG_\w+) (\d+)", header))
    assert int(limits["CRENDER_PHONG_MAX_LIGHTS"]) == capi.PHONG_MAX_LIGHTS == phong_ref.MAX_LIGHTS == 4
    assert 1 << int(limits["CRENDER_PHONG_MAX_SHININESS_LOG2"]) == capi.PHONG_MAX_SHININESS == 4096
    assert phong_ref.MAX_SHININESS_LOG2 == 12
    assert capi.ABI_VERSION == 6


def test_phong_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit_in_build(_build, "phong", ["phong.hip"], [os.path.join(INCLUDE, "crender_phong.h")])
    # the kernel takes the rasterizer's arithmetic and the passes' frame from the shared headers by inclusion
    unit = open(os.path.join(_build.SRC_DIR, "phong.hip")).read()
    # (the gather and the projection of the winner's corners are the header's winner_triangle)
    for name in ("winner_triangle(", "barycentric(", "guro_factor(", "make_proj(", "wave_any(", "winner_pixel(", "pass_grid("):
        assert name in unit and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name


def test_phong_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    nan, inf = float("nan"), float("inf")
    white = (C.c_float * 3)(255.0, 255.0, 255.0)

    def rows(*lights):
        return (C.c_float * (5 * len(lights)))(*[v for l in lights for v in l])
    one = rows((0.0, 0.0, -1.0, 0.9, 0.5))

    def shade(win=fake, tri=fake, T=4, pos_of=None, P=P, nrm=fake, lights=one, n=1, mask=0, ambient=0.1, k=5, spec=white,
              clamp=255.0, col=fake, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_phong_shade(win, tri, T, pos_of, P, nrm, lights, n, mask, ambient, k, spec, clamp, col,
                                     H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(P=None), dict(nrm=None), dict(lights=None), dict(spec=None), dict(col=None)):
        assert shade(**kw) == E and "is NULL" in text(), kw
    assert shade(tri=None) == E and "NULL with T > 0" in text()
    assert shade(T=-1) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2)):
        assert shade(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert shade(**kw) == E and "rows outside the frame" in text(), kw
    four = rows(*[(0.0, 0.0, -1.0, 0.9, 0.5)] * 4)
    for n in (0, 5, -1):
        assert shade(lights=four, n=n) == E and "n_lights is not 1 .. 4" in text(), n
    for n, mask in ((1, 2), (1, 3), (2, 4), (4, 16), (3, 0x80000000)):
        assert shade(lights=four, n=n, mask=mask) == E and "bits at or above n_lights" in text(), (n, mask)
    for k in (-1, 13, 32):
        assert shade(k=k) == E and "shininess_log2 is not 0 .. 12" in text(), k
    for bad in (nan, inf, -inf):
        assert shade(ambient=bad) == E and "not finite" in text(), bad
        for i in range(5):
            light = [0.0, 0.0, -1.0, 0.9, 0.5]
            light[i] = bad
            assert shade(lights=rows((0.0, 0.0, -1.0, 0.9, 0.5), light), n=2) == E and "not finite" in text(), (bad, i)
        for i in range(3):
            spec = [255.0] * 3
            spec[i] = bad
            assert shade(spec=(C.c_float * 3)(*spec)) == E and "not finite" in text(), (bad, i)
    assert shade(ambient=-0.001) == E and "negative" in text()
    for i in (3, 4):
        light = [0.0, 0.0, -1.0, 0.9, 0.5]
        light[i] = -0.5
        assert shade(lights=rows(light)) == E and "negative" in text(), i
    assert shade(clamp=nan) == E and "clamp is NaN" in text()
    for flags in (1, 2, 0x80000000):
        assert shade(flags=flags) == E and "unknown flag bits" in text(), flags
    assert text().startswith("crender_phong_shade")
    # a light beyond n_lights is not looked at; +inf is a clamp (none); without triangles there is nothing to launch
    assert shade(T=0, tri=None, lights=rows((0.0, 0.0, -1.0, 0.9, 0.5), (nan, nan, nan, -1.0, nan)), n=1) == capi.OK
    assert shade(T=0, clamp=inf) == capi.OK and shade(T=0, clamp=-inf) == capi.OK
    assert shade(T=0, mask=1) == capi.OK and shade(T=0, lights=four, n=4, mask=15) == capi.OK
    assert shade(T=0, k=13) == E


# ---- the model on the oracle's frame of T-Rex ------------------------------------------------------------------

class _Frame(Frame):
    def run(self, lights, **kw):
        return phong_ref.phong_pass(self.cam.color_buffer, self.cam.winner, self.tri, self.cam.proj_mat,
                                    self.cam.normals_buffer, lights, **kw)


trex = trex_fixture(_Frame)


def _point(pos=POINT, kd=0.9, ks=0.5):
    return dict(position=pos, diffuse=kd, specular=ks)


def test_one_directional_diffuse_light_is_guro(oracle, trex):
    got = trex.run([dict(direction=GURO, diffuse=1.0, specular=0.0)], ambient=0.0, clamp=np.inf)
    want = oracle.guro(trex.cam.color_buffer.copy(), trex.cam.normals_buffer, GURO)
    assert np.array_equal(got[trex.covered], want[trex.covered])            # as values: -0 against +0 is allowed
    assert_bit_equal(got[~trex.covered], trex.cam.color_buffer[~trex.covered], "the background is not written")
    assert (got[trex.covered] != trex.cam.color_buffer[trex.covered]).any()


@pytest.mark.parametrize("shininess,sp_pos,sp_half,clamped", [(1, 14589, 12046, 854), (32, 14586, 1078, 61),
                                                              (128, 12693, 318, 19)])
def test_the_counts_under_a_point_light(trex, shininess, sp_pos, sp_half, clamped):
    counts = {}
    out = trex.run([_point()], shininess=shininess, counts=counts)
    assert not np.isnan(out).any()
    assert counts["covered"] == 15801 and counts["clamped"] == clamped
    # The fall from 14 586 pixels with sp > 0 at shininess 32 to 12 693 at 128 is the squarings running through the
    # denormals to zero: a flush-to-zero build drops a factor as soon as it leaves the normal range and gets other counts.
    assert counts["lights"] == [dict(lit=14592, unlit=1209, sp_pos=sp_pos, sp_half=sp_half)]
    # what the scene is chosen for
    assert 1209 >= 0.05 * 15801 and clamped > 0
    if shininess == 32:
        assert sp_half >= 0.05 * 15801
    assert_bit_equal(out[~trex.covered], trex.cam.color_buffer[~trex.covered], "the background is not written")
    assert (out <= 255.0).all()


def test_the_second_light_leaves_a_third_unlit(trex):
    counts = {}
    out = trex.run([_point(), _point(SECOND)], counts=counts)
    assert not np.isnan(out).any()
    assert [(l["lit"], l["unlit"]) for l in counts["lights"]] == [(14592, 1209), (10273, 5528)]


def test_identities_bit_for_bit(trex):
    base = trex.cam.color_buffer
    # without a specular coefficient neither the exponent nor the highlight's colour matters
    a = trex.run([_point(ks=0.0), _point(SECOND, ks=0.0)], shininess=1, specular_color=(255, 255, 255))
    b = trex.run([_point(ks=0.0), _point(SECOND, ks=0.0)], shininess=4096, specular_color=(3, 200, 17))
    assert_bit_equal(a, b, "ks = 0")
    assert (a != base).any()
    # ambient 1 and no light: c * 1 + 0
    c = trex.run([_point(kd=0.0, ks=0.0)], ambient=1.0, clamp=np.inf)
    assert np.array_equal(c, base)
    # a second light with kd = ks = 0 adds +0 to both sums
    for first in (_point(), dict(direction=GURO, diffuse=0.7, specular=0.3)):
        one = trex.run([first])
        assert_bit_equal(trex.run([first, _point(SECOND, kd=0.0, ks=0.0)]), one, "a dark second light")
        assert_bit_equal(trex.run([first, dict(direction=(0, 1, 0), diffuse=0.0, specular=0.0)]), one, "a dark direction")
    # two lights in the other order: Ws is the same (0 + a + b), F differs by the rounding of a two-term sum only.
    # F < 2, so either order is within 2^-23 of the exact sum and the two within 2^-22 of each other: 6.1e-5 on a
    # colour of 255; the product c * F (below 512) and the final sum (below 1024) are rounded once each in either
    # order, 1.5e-5 and 3.1e-5 at the most per rounding: 1.6e-4 in all, below 2^-12
    x = trex.run([_point(), _point(SECOND)], clamp=np.inf)
    y = trex.run([_point(SECOND), _point()], clamp=np.inf)
    assert np.abs(x - y).max() <= 2.0 ** -12


def test_against_the_statements_in_float64(trex):
    """The same statements from the same float32 barycentrics in float64, at shininess 1 (the exponent multiplies a
    relative error, which is not what this test is about).  Measured on this frame: the largest absolute difference
    of a colour (values up to 255) is 4.47e-5.  The assertion is four times that, rounded up to a power of two,
    2^-12 = 2.44e-4: the margin is for other frames of the same scale.  It is a check of the model's statements, not
    a bound on the kernel, which is held to bit equality with the float32 model."""
    lights = [_point()]
    a = trex.run(lights, shininess=1)
    b = trex.run(lights, shininess=1, dtype=np.float64)
    assert a.dtype == np.float32 and b.dtype == np.float64
    diff = float(np.abs(a.astype(np.float64) - b).max())
    print(f"largest |float32 - float64| colour difference: {diff:.3e}")
    assert 0 < diff <= 2.0 ** -12


# ---- PhongIllumination -----------------------------------------------------------------------------------------

def test_phong_illumination_class():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, IlluminationDrawer, PhongIllumination
    from cython3dmodelrenderer_amd.illumination.phong_illumination import light_rows
    from cython3dmodelrenderer_amd.renderer import Renderer
    assert issubclass(PhongIllumination, IlluminationDrawer) and not hasattr(PhongIllumination, "fuse_into")
    p = PhongIllumination(direction=GURO)
    rows, mask = light_rows(p.lights)
    assert mask == 1 and len(rows) == 1
    assert_bit_equal(np.float32(rows[0][:3]), GuroIllumination(GURO).light_direction, "a direction's vector")
    assert np.float32(rows[0][3]) == np.float32(0.9) and np.float32(rows[0][4]) == np.float32(0.5)
    # the model and the class agree on the arguments of the C entry
    L5, m = phong_ref.lights5(p.lights + [dict(position=POINT, diffuse=0.25, specular=0.125)])
    rows, mask = light_rows(p.lights + [dict(position=POINT, diffuse=0.25, specular=0.125)])
    assert m == mask == 1
    assert_bit_equal(np.float32(rows), L5, "lights5")
    q = PhongIllumination(lights=[dict(position=POINT, diffuse=1, specular=0), dict(direction=GURO, diffuse=0.5, specular=0.5)])
    assert light_rows(q.lights)[1] == 2
    with pytest.raises(ValueError, match="exactly one of position and direction"):
        PhongIllumination()
    with pytest.raises(ValueError, match="exactly one of position and direction"):
        PhongIllumination(position=POINT, direction=GURO)
    with pytest.raises(ValueError, match="not both"):
        PhongIllumination(position=POINT, lights=[dict(position=POINT, diffuse=1, specular=0)])
    with pytest.raises(ValueError, match="1 to 4 dicts, got 5"):
        PhongIllumination(lights=[dict(position=POINT, diffuse=1, specular=0)] * 5)
    with pytest.raises(ValueError, match="1 to 4 dicts, got 0"):
        PhongIllumination(lights=[])
    with pytest.raises(ValueError, match="exactly one of 'position' and 'direction'"):
        PhongIllumination(lights=[dict(position=POINT, direction=GURO, diffuse=1, specular=0)])
    with pytest.raises(ValueError, match="power of two from 1 to 4096, got 48"):
        PhongIllumination(position=POINT, shininess=48)
    for bad in (0, 8192, 2.0, True):
        with pytest.raises(ValueError, match="power of two"):
            PhongIllumination(position=POINT, shininess=bad)
    with pytest.raises(ValueError, match="winner plane and the triangles.*on_device=None"):
        PhongIllumination(position=POINT).draw_illumination(np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 3), np.float32))

    class WithPass:
        def phong_pass(self):
            pass

    class Plain:
        pass
    for on_device in (False, "fused"):
        with pytest.raises(ValueError, match="PhongIllumination.*winner plane"):
            Renderer(WithPass(), PhongIllumination(position=POINT), on_device=on_device)
    with pytest.raises(ValueError, match="no phong_pass"):
        Renderer(Plain(), PhongIllumination(position=POINT))
    for on_device in (None, True):
        assert Renderer(WithPass(), PhongIllumination(position=POINT), on_device=on_device)._phong
    assert not Renderer(Plain(), GuroIllumination(GURO))._phong
