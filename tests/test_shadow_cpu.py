"""The shadow pass without a GPU: the header against the binding and the build lists, the entry point's argument
checks, the host model the GPU tests compare with (tests/shadow_ref.py) pinned by hand on a floor under an occluder
and on the oracle's frames of T-Rex, and the light-frame helpers of cython3dmodelrenderer_amd/shadow.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import shadow_ref
from pass_scenes import capi  # noqa: F401 (fixtures)
from util import INCLUDE, assert_bit_equal, other_symbols, unit_in_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_shadow_header_symbol_is_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_shadow.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["shadow"]) == {"crender_shadow_shade"}
    assert not declared & other_symbols(capi, "shadow")
    L = capi.load()
    assert L.crender_shadow_shade.argtypes == capi.UNIT_SIGNATURES["shadow"]["crender_shadow_shade"][1]
    # argument counts: the declaration's commas against the table
    decl = re.search(r"CRENDER_API int crender_shadow_shade\((.*?)\);", header, re.S).group(1)
    res, args = capi.UNIT_SIGNATURES["shadow"]["crender_shadow_shade"]
    assert res == C.c_int and len(args) == len(decl.split(",")) == 21
    # the three floats of the declaration are the table's: bias and ambient by value, the matrices as host pointers
    kinds = ["float" if re.match(r"\s*float \w+$", a) else "other" for a in decl.split(",")]
    assert [i for i, k in enumerate(kinds) if k == "float"] == [i for i, a in enumerate(args) if a is C.c_float] == [11, 12]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    assert capi.SHADOW_PCF == shadow_ref.PCF == (1, 3, 5)
    assert capi.ABI_VERSION == 6


def test_shadow_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit_in_build(_build, "shadow", ["shadow.hip"], [os.path.join(INCLUDE, "crender_shadow.h")])
    # the kernel takes the rasterizer's arithmetic from the fingerprinted headers by inclusion
    unit = open(os.path.join(_build.SRC_DIR, "shadow.hip")).read()
    for name in ("project_vertex(", "barycentric(", "make_proj(", "wave_any("):
        assert name in unit and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name


def test_shadow_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    nan, inf = float("nan"), float("inf")

    def shade(win=fake, tri=fake, T=4, pos_of=None, P=P, ltri=fake, PL=P, lz=fake, lwin=None, Hl=8, Wl=8, bias=1e-3,
              ambient=0.25, pcf=1, col=fake, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_shadow_shade(win, tri, T, pos_of, P, ltri, PL, lz, lwin, Hl, Wl, bias, ambient, pcf, col,
                                      H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(P=None), dict(PL=None), dict(lz=None), dict(col=None)):
        assert shade(**kw) == E and "NULL" in text(), kw
    for kw in (dict(tri=None), dict(ltri=None)):
        assert shade(**kw) == E and "NULL with T > 0" in text(), kw
    assert shade(T=-1) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2)):
        assert shade(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(Hl=0), dict(Wl=-1)):
        assert shade(**kw) == E and "Hl or Wl is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert shade(**kw) == E and "rows outside the frame" in text(), kw
    for pcf in (0, 2, 4, 7, -1):
        assert shade(pcf=pcf) == E and "pcf is not 1, 3 or 5" in text(), pcf
    for ambient in (-0.001, 1.001, nan, inf):
        assert shade(ambient=ambient) == E and "ambient outside [0, 1] or NaN" in text(), ambient
    for bias in (nan, inf, -inf):
        assert shade(bias=bias) == E and "bias is not finite" in text(), bias
    for flags in (1, 2, 0x80000000):
        assert shade(flags=flags) == E and "unknown flag bits" in text(), flags
    assert text().startswith("crender_shadow_shade")
    # without triangles there is nothing to launch, and the triangle arrays may be missing
    assert shade(T=0, tri=None, ltri=None) == capi.OK
    assert shade(T=0, pcf=2) == E


# ---- the model by hand: a floor under a smaller occluder ---------------------------------------------------------

def _quad(x0, x1, y0, y1, z):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return np.float32([[a, b, c], [a, c, d]])


def _floor_and_occluder(oracle):
    """Camera and light both look down +z at fov 90 on 8 x 8 frames, so a point (X, Y, Z) lands on pixel
    ((X / Z + 1) * 4, (Y / Z + 1) * 4), in powers of two throughout.  The floor (triangles 0, 1) is the plane z = 2
    across the whole view; the light stands one unit to the left of the camera (t = (1, 0, 0)), which moves the floor
    by TWO texels: the camera's floor pixel (x, y) is the light's texel (x + 2, y).  The occluder (triangles 2, 3) is
    the rectangle [-1.1, -0.6] x [-0.35, 0.1] of the plane z = 1: the camera's pixels x = 0, 1 of rows 3, 4 and,
    moved by FOUR texels at that depth, the light's texels x = 4, 5 of the same rows."""
    from cython3dmodelrenderer_amd import shadow
    tri = np.concatenate([_quad(-2.5, 2.5, -2.5, 2.5, 2.0), _quad(-1.1, -0.6, -0.35, 0.1, 1.0)])
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1
    col = np.random.default_rng(5).uniform(10, 250, tri.shape).astype(np.float32)
    ltri, lnrm = shadow.light_arrays(tri, nrm, np.eye(3, dtype=np.float32), np.float32([1, 0, 0]))
    cam = oracle.OracleFiller(8, 8, fov=90.0)
    cam.render_arrays(tri, col, nrm)
    lig = oracle.OracleFiller(8, 8, fov=90.0)
    lig.render_arrays(ltri, col, lnrm)
    return tri, ltri, cam, lig


def test_the_model_by_hand_on_a_floor_under_an_occluder(oracle):
    d = np.float32
    tri, ltri, cam, lig = _floor_and_occluder(oracle)
    occluder = np.zeros((8, 8), bool)
    occluder[3:5, 0:2] = True
    assert ((cam.winner >= 2) == occluder).all() and (cam.winner >= 0).all()
    seen = np.zeros((8, 8), bool)
    seen[3:5, 4:6] = True
    assert ((lig.winner >= 2) == seen).all()
    assert (lig.winner[:, 0] == -1).all() and (lig.winner[:, 1:] >= 0).all()   # the floor ends at the light's column 1

    def run(**kw):
        return shadow_ref.shadow_pass(cam.color_buffer, cam.winner, tri, cam.proj_mat, ltri, lig.proj_mat, lig.z_buffer,
                                      bias=1e-3, ambient=0.25, **kw)

    # K = 1: the floor pixels whose texel (x + 2, y) the occluder took, x = 2, 3 of rows 3, 4, keep `ambient` of
    # their colour; the occluder itself, the floor elsewhere, and the columns 6, 7 whose texel is off the map, are
    # not touched
    want = cam.color_buffer.copy()
    want[3:5, 2:4] = want[3:5, 2:4] * d(0.25)
    for lwinner in (None, lig.winner):
        assert_bit_equal(run(pcf=1, lwinner=lwinner), want, "K = 1")
    # K = 3: a floor pixel loses one ninth per tap inside the occluder's texels: columns x + 2 + i in {4, 5} for
    # 1, 2, 2, 1 of the three i at x = 1, 2, 3, 4, rows y + j in {3, 4} for 1, 2, 2, 1 of the three j at y = 2 .. 5
    across = np.array([0, 1, 2, 2, 1, 0, 0, 0])
    down = np.array([0, 0, 1, 2, 2, 1, 0, 0])
    n = 9 - down[:, None] * across[None, :]
    n[occluder] = 9                    # nearer than everything around it
    assert n.min() == 5 and (n[3:5, 2:4] == 5).all() and n[2, 1] == 8 and n[3, 4] == 7
    f = d(0.25) + d(0.75) * (n.astype(np.float32) / d(9))
    want = np.where((n < 9)[:, :, None], cam.color_buffer * f[:, :, None], cam.color_buffer)
    for lwinner in (None, lig.winner):
        assert_bit_equal(run(pcf=3, lwinner=lwinner), want, "K = 3")
    # K = 5 reaches one texel further, and the taps beyond the map's edge count as lit
    counts = {}
    got = run(pcf=5, counts=counts)
    touched = (got.view(np.uint32) != cam.color_buffer.view(np.uint32)).any(2)
    assert touched[1:7, 0:6].sum() == 36 - 4 and not touched[:, 6:].any() and not touched[[0, 7]].any()
    assert counts == {"covered": 64, "lit": 32, "shadowed": 0}


def test_without_a_bias_only_the_winner_rule_keeps_a_surface_from_shadowing_itself(oracle):
    tri, ltri, cam, lig = _floor_and_occluder(oracle)
    kw = dict(bias=0.0, ambient=0.0, pcf=1)
    plain, ruled = {}, {}
    shadow_ref.shadow_pass(cam.color_buffer, cam.winner, tri, cam.proj_mat, ltri, lig.proj_mat, lig.z_buffer,
                           counts=plain, **kw)
    out = shadow_ref.shadow_pass(cam.color_buffer, cam.winner, tri, cam.proj_mat, ltri, lig.proj_mat, lig.z_buffer,
                                 lig.winner, counts=ruled, **kw)
    # the depth a pixel carries into the map and the depth the light's filler stored there are two roundings of one
    # number: without a bias some of the floor shadows itself (acne), with the winner rule only the true shadow stays
    assert plain["shadowed"] > 4 and ruled["shadowed"] == 4 and ruled["lit"] == 60
    assert (out[3:5, 2:4] == 0).all() and (out != 0).any(2).sum() == 60


def test_nan_and_the_far_side_of_the_light_are_lit(oracle):
    tri, ltri, cam, lig = _floor_and_occluder(oracle)
    args = (cam.color_buffer, cam.winner, tri, cam.proj_mat)
    # a NaN or cleared map, a NaN light-frame point, a light with the scene behind it: nothing is written
    for lz in (np.full((8, 8), np.nan, np.float32), np.full((8, 8), 1e6, np.float32), np.full((8, 8), np.inf, np.float32)):
        assert_bit_equal(shadow_ref.shadow_pass(*args, ltri, lig.proj_mat, lz), cam.color_buffer, "map")
    assert_bit_equal(shadow_ref.shadow_pass(*args, ltri * np.float32(np.nan), lig.proj_mat, lig.z_buffer), cam.color_buffer, "NaN")
    assert_bit_equal(shadow_ref.shadow_pass(*args, ltri - np.float32([0, 0, 5]), lig.proj_mat, lig.z_buffer), cam.color_buffer, "behind")
    # while a map that holds -inf shadows every pixel whose texel is on it: the columns 0 .. 5
    out = shadow_ref.shadow_pass(*args, ltri, lig.proj_mat, np.full((8, 8), -np.inf, np.float32), ambient=0.5)
    assert_bit_equal(out[:, :6], cam.color_buffer[:, :6] * np.float32(0.5), "-inf")
    assert_bit_equal(out[:, 6:], cam.color_buffer[:, 6:], "off the map")


# ---- the light's frame -------------------------------------------------------------------------------------------

def test_look_at_is_orthonormal_and_looks_down_plus_z():
    from cython3dmodelrenderer_amd import shadow
    R, t = shadow.look_at((0, 0, 0), (0, 0, 5))
    assert R.dtype == t.dtype == np.float32 and np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
    rng = np.random.default_rng(1)
    for _ in range(20):
        pos, target = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
        R, t = shadow.look_at(pos, target)
        assert R.shape == (3, 3) and t.shape == (3,) and R.dtype == t.dtype == np.float32
        assert np.abs(R.astype(np.float64) @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-6
        assert np.abs(R @ pos.astype(np.float32) + t).max() < 1e-5                  # the light sits at its origin
        ahead = R.astype(np.float64) @ target + t
        assert abs(ahead[0]) < 1e-5 and abs(ahead[1]) < 1e-5 and abs(ahead[2] - np.linalg.norm(target - pos)) < 1e-5
        assert (R.astype(np.float64) @ np.array([0, -1, 0]))[1] < 0                 # `up` points to smaller rows
    with pytest.raises(ValueError, match="coincide"):
        shadow.look_at((1, 2, 3), (1, 2, 3))
    with pytest.raises(ValueError, match="parallel"):
        shadow.look_at((0, 0, 0), (0, 2, 0))


def test_light_arrays_against_a_float64_evaluation_in_numpy_and_torch():
    import torch
    from cython3dmodelrenderer_amd import scenes, shadow
    tri, _, nrm = scenes.load_fixture("trex_inputs.npz")
    R, t = shadow.look_at((1.5, -2.0, -0.5), (0, 0, 1))
    ltri, lnrm = shadow.light_arrays(tri, nrm, R, t)
    assert ltri.dtype == lnrm.dtype == np.float32 and ltri.shape == lnrm.shape == tri.shape and ltri.flags.c_contiguous
    R64 = R.astype(np.float64)
    # three products and three sums of numbers below 4, each rounded to float32: a few units of 2^-24 * 4
    assert np.abs(ltri - (tri.astype(np.float64) @ R64.T + t)).max() < 2e-6
    assert np.abs(lnrm - nrm.astype(np.float64) @ R64.T).max() < 2e-6
    # the statement is spelled out per operation, so torch gives the same bits
    a, b = shadow.light_arrays(torch.from_numpy(tri), torch.from_numpy(nrm), R, t)
    assert isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.is_contiguous()
    assert_bit_equal(a.numpy(), ltri, "vertices")
    assert_bit_equal(b.numpy(), lnrm, "normals")
    # a strided view is taken as it is
    c, _ = shadow.light_arrays(tri[::2], nrm[::2], R, t)
    assert_bit_equal(c, ltri[::2], "strided")


def test_renderer_refuses_a_filler_without_a_shadow_pass():
    from cython3dmodelrenderer_amd.renderer import Renderer

    class Plain:
        pass
    with pytest.raises(ValueError, match="no shadow_pass"):
        Renderer(Plain(), None, shadow={"filler": None, "R": np.eye(3), "t": np.zeros(3)})

    class Shadowing:
        def shadow_pass(self):
            pass
    with pytest.raises(ValueError, match="'t'.*missing"):
        Renderer(Shadowing(), None, shadow={"filler": None, "R": np.eye(3)})
    assert Renderer(Plain(), None).shadow is None


# ---- the oracle's frames of T-Rex --------------------------------------------------------------------------------

def test_the_measured_figures_on_the_oracles_frames_of_trex(oracle):
    """T-Rex at 256 x 256 and a 256 x 256 map, both fov 45, K = 1.  The light's frame holds the model turned about
    the float32 mean of its corners by the y block [[cos 40, -sin 40], [sin 40, cos 40]] — ``Model.rotate((0, -40, 0))``
    in that method's own sign convention, which is what gives the figures this pass was specified with:

        bias   winner rule   covered   fully lit   fully shadowed
        1e-3   no            15 801    88.1 %      11.9 %       (with the rule 11 pixels more are lit: 88.2 %)
        0      no            15 801    48.3 %      51.7 %
        0      yes           15 801    78.8 %      21.2 %
    """
    from cython3dmodelrenderer_amd import scenes, shadow
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    R, t = shadow_ref.rotation_frame(tri, (0, -40, 0))
    ltri, lnrm = shadow.light_arrays(tri, nrm, R, t)
    cam = oracle.OracleFiller(256, 256, fov=45.0)
    cam.render_arrays(tri, col, nrm)
    lig = oracle.OracleFiller(256, 256, fov=45.0)
    lig.render_arrays(ltri, col, lnrm)

    def count(bias, lwinner, ref=cam, ltri=ltri, PL=lig.proj_mat, lz=lig.z_buffer):
        c = {}
        shadow_ref.shadow_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, ltri, PL, lz, lwinner, bias=bias, counts=c)
        assert c["covered"] == 15801 and c["lit"] + c["shadowed"] == 15801         # K = 1: nothing in between
        return round(100.0 * c["lit"] / 15801, 1), round(100.0 * c["shadowed"] / 15801, 1), c["lit"]

    assert count(1e-3, None)[:2] == (88.1, 11.9)
    assert count(1e-3, lig.winner)[:2] == (88.2, 11.8) and count(1e-3, lig.winner)[2] - count(1e-3, None)[2] == 11
    assert count(0.0, None)[:2] == (48.3, 51.7)
    assert count(0.0, lig.winner)[:2] == (78.8, 21.2)
    # the light at the camera: the frame's own planes as the map
    own = dict(ltri=tri, PL=cam.proj_mat, lz=cam.z_buffer)
    assert count(0.0, cam.winner, **own)[2] == 15801
    assert count(0.0, None, **own)[2] == 10703
    assert count(1e-5, None, **own)[2] == 15801
