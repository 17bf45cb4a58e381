"""Every instance of every deferred pass over the hand-built scenes of tests/pass_edges.py, through the C entry points
(crender_tex_shade, crender_mip_shade, crender_aniso_shade, crender_shadow_shade, crender_phong_shade,
crender_ao_shade, crender_wire_overlay, crender_wire_outline) on planes the test allocates itself:
the rasterizer is not involved, so the kernels meet winners that do not contain their pixel, triangles of no area and
of 10^13 px^2, corners at z = 2^-43, 2^40 or NaN, and take both sides of every window decision of the shared-reciprocal
shortcut (tests/test_pass_edges_cpu.py counts them).  Bit for bit against the host models; where a model's colour is
a NaN the kernel's must be one.

The two wire kernels, after the occlusion pass: every instance on the painted scene, then the outline alone on the frame
that holds its depth test at equality and on the frames of lone winners, where a wavefront that skips a row too many,
or a halo a pixel too narrow, leaves a pixel unlit."""
import ctypes as C

import numpy as np
import pytest

import aniso_ref
import ao_ref
import mip_ref
import outline_ref
import overlay_ref
import pass_edges as E
import phong_ref
import shadow_ref
import tex_ref
from pass_scenes import lib, light3, stream  # noqa: F401 (lib is a fixture)
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

AMBIENT = 0.25
ROWS = (5, 77)                       # a strip whose ends are no multiples of 8


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: {int((np.isnan(got) != nan).sum())} pixels differ in NaN-ness"
    zero = np.float32(0)
    assert_bit_equal(np.where(nan, zero, got), np.where(nan, zero, want), what)


class _Device:
    """A scene's arrays on the device, and the host copies they must still equal afterwards."""

    def __init__(self, s):
        self.s = s
        self.kept = {k: getattr(s, k) for k in ("winner", "tri", "uv", "ltri", "normals", "lz", "lwinner", "z") if hasattr(s, k)}
        for k, v in self.kept.items():
            setattr(self, k, _dev(v))
        if hasattr(s, "pos_of"):
            self.moved, self.pos_of = _dev(s.moved), _dev(s.pos_of.view(np.int32))

    def untouched(self, what):
        for k, v in self.kept.items():
            assert_bit_equal(getattr(self, k).cpu().numpy(), v, f"{what}: the pass wrote to {k}")


class _Texture:
    def __init__(self, lib, name, tex):
        import torch
        from cython3dmodelrenderer_amd import _capi
        self.name, self.tex = name, tex
        self.th, self.tw = tex.shape[:2]
        self.chain = mip_ref.build_chain(tex)
        self.d_tex = _dev(tex)
        self.d_chain = torch.empty(mip_ref.layout(self.th, self.tw)[2], dtype=torch.uint8, device="cuda")
        _capi.check(lib.crender_mip_build(self.d_tex.data_ptr(), self.th, self.tw, self.d_chain.data_ptr(), stream()),
                    "crender_mip_build")


SHAPES = {"1x1": (1, 1), "3x1000": (3, 1000), "64x97": (64, 97), "1x65535": (1, 65535), "40000x2": (40000, 2)}


@pytest.fixture(scope="module")
def textures(lib):
    rng = np.random.default_rng(20243)
    return {name: _Texture(lib, name, rng.integers(0, 256, (th, tw, 3), dtype=np.uint8)) for name, (th, tw) in SHAPES.items()}


@pytest.fixture(scope="module")
def edge(oracle):
    return _Device(E.scene())


@pytest.fixture(scope="module")
def mini(oracle):
    return _Device(E.mini_scene())


@pytest.fixture(scope="module")
def tall(oracle):
    return _Device(E.tall_scene())


def _texture_family(lib, oracle, D, kind, tx, persp, light, y0=0, y1=None, pos_of=False, bilinear=False, A=1):
    """(got, want): one call of a texture entry on a fresh copy of the scene's colour plane, and the host model's answer."""
    from cython3dmodelrenderer_amd import _capi
    s = D.s
    y1 = s.H if y1 is None else y1
    color = _dev(s.color)
    head = (D.winner.data_ptr(), (D.moved if pos_of else D.tri).data_ptr(), s.T, D.pos_of.data_ptr() if pos_of else None,
            _capi.f32_16(E.P), D.uv.data_ptr())
    tail = (D.normals.data_ptr() if light else None, light3(oracle) if light else None, color.data_ptr(), s.H, s.W, y0, y1)
    winner = s.winner_without_gone if pos_of else s.winner
    lit = dict(normals=s.normals, light_direction=E.LIGHT) if light else {}
    if kind == "tex":
        flags = (_capi.TEX_PERSPECTIVE if persp else 0) | (_capi.TEX_BILINEAR if bilinear else 0)
        _capi.check(lib.crender_tex_shade(*head, tx.d_tex.data_ptr(), tx.th, tx.tw, *tail, flags, stream()), "crender_tex_shade")
        want = tex_ref.texture_pass(s.color, winner, s.tri, E.P, s.uv, tx.tex, persp, bilinear, y0=y0, y1=y1, **lit)
    elif kind == "mip":
        _capi.check(lib.crender_mip_shade(*head, tx.d_chain.data_ptr(), tx.th, tx.tw, *tail, _capi.MIP_PERSPECTIVE if persp else 0,
                                          stream()), "crender_mip_shade")
        want = mip_ref.texture_pass(s.color, winner, s.tri, E.P, s.uv, None, persp, y0=y0, y1=y1, chain=tx.chain, **lit)
    else:
        _capi.check(lib.crender_aniso_shade(*head, tx.d_chain.data_ptr(), tx.th, tx.tw, *tail, _capi.MIP_PERSPECTIVE if persp else 0,
                                            A, stream()), "crender_aniso_shade")
        want = aniso_ref.texture_pass(s.color, winner, s.tri, E.P, s.uv, None, persp, A, y0=y0, y1=y1, chain=tx.chain, **lit)
    return color.cpu().numpy(), want


def _every_variant(lib, oracle, D, textures, kind, what, **kw):
    """The whole frame under every texture, then a strip of rows and d_pos_of under the 64 x 97 one."""
    changed = 0
    for tx in textures.values():
        got, want = _texture_family(lib, oracle, D, kind, tx, **kw)
        _same(got, want, f"{what}, texture {tx.name}")
        changed += int((want.view(np.uint32) != D.s.color.view(np.uint32)).any(2).sum())
    assert changed > 5 * 5000
    tx = textures["64x97"]
    y0, y1 = ROWS
    got, want = _texture_family(lib, oracle, D, kind, tx, y0=y0, y1=y1, **kw)
    assert_bit_equal(got[:y0], D.s.color[:y0], f"{what}: rows above the strip")
    assert_bit_equal(got[y1:], D.s.color[y1:], f"{what}: rows below the strip")
    _same(got, want, f"{what}, rows {y0} .. {y1}")
    got, want = _texture_family(lib, oracle, D, kind, tx, pos_of=True, **kw)
    _same(got, want, f"{what}, d_pos_of")
    gone = D.s.winner == D.s.gone
    if not kw["light"]:
        assert_bit_equal(got[gone], D.s.color[gone], f"{what}: a triangle d_pos_of sends beyond T is background")
    D.untouched(what)


# ---- crender_mip_build -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SHAPES))
def test_mip_build_matches_the_model(textures, name):
    tx = textures[name]
    assert len(tx.chain) == {"1x1": 1, "3x1000": 10, "64x97": 7, "1x65535": 16, "40000x2": 16}[name]
    assert_bit_equal(tx.d_chain.cpu().numpy(), mip_ref.pack_chain(tx.chain), f"the chain of a {name} texture")
    assert_bit_equal(tx.d_tex.cpu().numpy(), tx.tex, "the texture is only read")


# ---- the edge scene ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("persp", [False, True])
def test_tex_shade_every_instance(lib, oracle, edge, textures, persp, bilinear, light):
    _every_variant(lib, oracle, edge, textures, "tex", f"tex persp={persp} bilinear={bilinear} light={light}",
                   persp=persp, bilinear=bilinear, light=light)


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("persp", [False, True])
def test_mip_shade_every_instance(lib, oracle, edge, textures, persp, light):
    _every_variant(lib, oracle, edge, textures, "mip", f"mip persp={persp} light={light}", persp=persp, light=light)


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 16])
@pytest.mark.parametrize("persp", [False, True])
def test_aniso_shade_every_instance(lib, oracle, edge, textures, persp, A, light):
    _every_variant(lib, oracle, edge, textures, "aniso", f"aniso persp={persp} A={A} light={light}", persp=persp, A=A, light=light)
    if A == 1:
        for tx in textures.values():
            a, _ = _texture_family(lib, oracle, edge, "aniso", tx, persp=persp, light=light, A=1)
            m, _ = _texture_family(lib, oracle, edge, "mip", tx, persp=persp, light=light)
            _same(a, m, f"max_aniso = 1 against crender_mip_shade, persp={persp} light={light}, texture {tx.name}")


def _shadow(lib, D, K, use_winner, y0=0, y1=None, pos_of=False, ambient=AMBIENT):
    from cython3dmodelrenderer_amd import _capi
    s = D.s
    y1 = s.H if y1 is None else y1
    color = _dev(s.color)
    Hl, Wl = s.lz.shape
    _capi.check(lib.crender_shadow_shade(
        D.winner.data_ptr(), (D.moved if pos_of else D.tri).data_ptr(), s.T, D.pos_of.data_ptr() if pos_of else None,
        _capi.f32_16(E.P), D.ltri.data_ptr(), _capi.f32_16(E.P), D.lz.data_ptr(), D.lwinner.data_ptr() if use_winner else None,
        Hl, Wl, E.BIAS, ambient, K, color.data_ptr(), s.H, s.W, y0, y1, 0, stream()), "crender_shadow_shade")
    want = shadow_ref.shadow_pass(s.color, s.winner_without_gone if pos_of else s.winner, s.tri, E.P, s.ltri, E.P, s.lz,
                                  s.lwinner if use_winner else None, bias=E.BIAS, ambient=ambient, pcf=K, y0=y0, y1=y1)
    return color.cpu().numpy(), want


@pytest.mark.parametrize("use_winner", [False, True])
@pytest.mark.parametrize("K", [1, 3, 5])
def test_shadow_shade_every_instance(lib, oracle, edge, K, use_winner):
    what = f"shadow K={K} use_winner={use_winner}"
    s = edge.s
    got, want = _shadow(lib, edge, K, use_winner)
    assert not np.isnan(want).any()                  # every NaN is lit: none reaches the colours
    _same(got, want, what)
    assert (want.view(np.uint32) != s.color.view(np.uint32)).any(2).sum() > 500
    y0, y1 = ROWS
    got, want = _shadow(lib, edge, K, use_winner, y0=y0, y1=y1)
    assert_bit_equal(got[:y0], s.color[:y0], f"{what}: rows above the strip")
    assert_bit_equal(got[y1:], s.color[y1:], f"{what}: rows below the strip")
    _same(got, want, f"{what}, rows {y0} .. {y1}")
    got, want = _shadow(lib, edge, K, use_winner, pos_of=True)
    _same(got, want, f"{what}, d_pos_of")
    gone = s.winner == s.gone
    assert_bit_equal(got[gone], s.color[gone], f"{what}: a triangle d_pos_of sends beyond T is background")
    for ambient in (0.0, 1.0):
        got, want = _shadow(lib, edge, K, use_winner, ambient=ambient)
        _same(got, want, f"{what}, ambient {ambient}")
    edge.untouched(what)


def _phong(lib, D, lights, shininess=32, y0=0, y1=None, pos_of=False, ambient=AMBIENT, clamp=255.0, spec=(255.0, 200.0, 17.5)):
    """(got, want): one call of crender_phong_shade on a fresh copy of the scene's colour plane, and the host model's."""
    from cython3dmodelrenderer_amd import _capi
    s = D.s
    y1 = s.H if y1 is None else y1
    color = _dev(s.color)
    L5, mask = phong_ref.lights5(lights)
    _capi.check(lib.crender_phong_shade(
        D.winner.data_ptr(), (D.moved if pos_of else D.tri).data_ptr(), s.T, D.pos_of.data_ptr() if pos_of else None,
        _capi.f32_16(E.P), D.normals.data_ptr(), (C.c_float * L5.size)(*L5.reshape(-1).tolist()), len(lights), mask, ambient,
        int(shininess).bit_length() - 1, (C.c_float * 3)(*spec), clamp, color.data_ptr(), s.H, s.W, y0, y1, 0, stream()),
        "crender_phong_shade")
    want = phong_ref.phong_pass(s.color, s.winner_without_gone if pos_of else s.winner, s.tri, E.P, s.normals, lights,
                                ambient=ambient, shininess=shininess, specular_color=spec, clamp=clamp, y0=y0, y1=y1)
    return color.cpu().numpy(), want


@pytest.mark.parametrize("shininess", [1, 32, 4096])
@pytest.mark.parametrize("kind", E.LIGHT_SETS)
def test_phong_shade_every_instance(lib, oracle, edge, kind, shininess):
    """One light runs the instance without the loop frame, four the loop; 0, 5 and 12 squarings.  The pixels outside
    their winner, the triangles of no area and the corners at z = 0, NaN and +-inf all end as finite colours
    (tests/test_pass_edges_cpu.py), so every comparison is of bits."""
    what = f"phong {kind} shininess={shininess}"
    s = edge.s
    lights = s.lights[kind]
    got, want = _phong(lib, edge, lights, shininess)
    assert np.isfinite(want).all()
    _same(got, want, what)
    covered = (s.winner >= 0) & (s.winner < s.T)
    assert (want.view(np.uint32) != s.color.view(np.uint32)).any(2)[covered].all()
    assert_bit_equal(got[~covered], s.color[~covered], f"{what}: the background and the pixels of bad winners")
    y0, y1 = ROWS
    got, want = _phong(lib, edge, lights, shininess, y0=y0, y1=y1)
    assert_bit_equal(got[:y0], s.color[:y0], f"{what}: rows above the strip")
    assert_bit_equal(got[y1:], s.color[y1:], f"{what}: rows below the strip")
    _same(got, want, f"{what}, rows {y0} .. {y1}")
    got, want = _phong(lib, edge, lights, shininess, pos_of=True)
    _same(got, want, f"{what}, d_pos_of")
    gone = s.winner == s.gone
    assert_bit_equal(got[gone], s.color[gone], f"{what}: a triangle d_pos_of sends beyond T is background")
    for kw in (dict(ambient=0.0), dict(clamp=float("inf")), dict(clamp=100.0)):
        got, want = _phong(lib, edge, lights, shininess, **kw)
        _same(got, want, f"{what}, {kw}")
    assert (want == np.float32(100)).any(2).sum() >= 16
    edge.untouched(what)


def _ao(lib, D, table, face, rotate, radius_px, radius, y0=0, y1=None, pos_of=False, want_pos_of=None, strength=2.0, floor=0.0):
    """(got, want): one call of crender_ao_shade on a fresh copy of the scene's colour plane, and the host model's.
    `pos_of` hands the kernel d_pos_of and the moved triangles; `want_pos_of` (by default the same) the model."""
    from cython3dmodelrenderer_amd import _capi
    s = D.s
    y1 = s.H if y1 is None else y1
    color = _dev(s.color)
    taps2 = (C.c_int8 * (2 * len(table)))(*[v for p in table for v in p])
    flags = (_capi.AO_ROTATE if rotate else 0) | (_capi.AO_FACE_NORMALS if face else 0)
    _capi.check(lib.crender_ao_shade(
        D.winner.data_ptr(), D.z.data_ptr(), (D.moved if pos_of else D.tri).data_ptr(), s.T,
        D.pos_of.data_ptr() if pos_of else None, _capi.f32_16(E.P), D.normals.data_ptr(), taps2, len(table), radius_px, radius,
        0.1, strength, floor, color.data_ptr(), s.H, s.W, y0, y1, flags, stream()), "crender_ao_shade")
    model_pos_of = pos_of if want_pos_of is None else want_pos_of
    counts = {}
    want = ao_ref.ao_pass(s.color, s.z, s.winner, s.moved if model_pos_of else s.tri, E.P, s.normals, table, radius=radius,
                          radius_px=radius_px, min_cos=0.1, strength=strength, floor=floor, rotate=rotate, face=face,
                          pos_of=s.pos_of if model_pos_of else None, T=s.T, y0=y0, y1=y1, counts=counts)
    assert not np.isnan(want).any() and counts["occluded"] > 0
    return color.cpu().numpy(), want


def _ao_table(s, radius_px):
    """(table, radius): every neighbour at 1 px, tests/test_ao_gpu.py's 16 taps at 8, and at 32 the corners and the
    edges of the halo as well, under a radius that reaches them."""
    from cython3dmodelrenderer_amd import ambient_occlusion
    return {1: (ambient_occlusion.taps(1, 8), s.ao_radius), 8: (E.TABLE, s.ao_radius),
            32: (E.HALO_TABLE + E.TABLE, s.halo_radius)}[radius_px]


@pytest.mark.parametrize("radius_px", [1, 8, 32])
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("face", [False, True])
def test_ao_shade_on_the_edge_scene(lib, oracle, edge, face, rotate, radius_px):
    """Face normals of triangles whose cross product is inf, 0 or NaN, a z plane with NaN, +-inf and the division by
    zero, bad winners in the halo; a strip of rows 5 .. 77 on a frame of less than three tiles of 32 with up to 32 px
    of halo on every side."""
    what = f"ao face={face} rotate={rotate} radius_px={radius_px}"
    s = edge.s
    table, radius = _ao_table(s, radius_px)
    got, want = _ao(lib, edge, table, face, rotate, radius_px, radius)
    _same(got, want, what)
    y0, y1 = ROWS
    got, want = _ao(lib, edge, table, face, rotate, radius_px, radius, y0=y0, y1=y1)
    assert_bit_equal(got[:y0], s.color[:y0], f"{what}: rows above the strip")
    assert_bit_equal(got[y1:], s.color[y1:], f"{what}: rows below the strip")
    _same(got, want, f"{what}, rows {y0} .. {y1}")             # (the model does not look across the strip's edge)
    if face:
        got, want = _ao(lib, edge, table, face, rotate, radius_px, radius, pos_of=True)
        _same(got, want, f"{what}, d_pos_of")
        gone = s.winner == s.gone
        assert_bit_equal(got[gone], s.color[gone], f"{what}: a triangle d_pos_of sends beyond T is not written")
        # `s > 0`, not `s >= 0`: under a radius that takes every tap (tests/test_pass_edges_cpu.py counts the pixels)
        got, want = _ao(lib, edge, table, face, rotate, radius_px, 1e30)
        _same(got, want, f"{what}, radius 1e30")
    else:
        got, want = _ao(lib, edge, table, face, rotate, radius_px, radius, pos_of=True, want_pos_of=False)
        _same(got, want, f"{what}: the plane mode does not look at d_pos_of")
    got, want = _ao(lib, edge, table, face, rotate, radius_px, radius, strength=50.0, floor=0.25)
    _same(got, want, f"{what}, strength 50 over a floor")
    edge.untouched(what)


# ---- the wire passes ----------------------------------------------------------------------------------------------------

LINE = (250.0, 240.0, 20.0)
FILL = (30.0, 35.0, 40.0)
WIDE = dict(width=64.0, feather=64.0)            # hi / feather is 1: the ramp everywhere, the cap on a line alone
_FIELDS = {}                                     # the outline model's distance fields: they do not depend on the style


def _wire(lib, D, outline, fill=None, masked=False, y0=0, y1=None, pos_of=False, width=1.0, feather=1.0, opacity=1.0,
          depth_bias=1e-3, radius_px=2):
    """(got, want): one call of crender_wire_overlay or crender_wire_outline on a fresh copy of the scene's colour
    plane, and the host model's answer, which must hold no NaN.  `masked`: the scene's edge mask, in the caller's order
    with and without d_pos_of."""
    from cython3dmodelrenderer_amd import _capi
    s = D.s
    y1 = s.H if y1 is None else y1
    color = _dev(s.color)
    if not hasattr(D, "edges"):
        D.edges = _dev(s.edges)
    head = ((D.moved if pos_of else D.tri).data_ptr(), s.T, D.pos_of.data_ptr() if pos_of else None, _capi.f32_16(E.P),
            D.edges.data_ptr() if masked else None, (C.c_float * 3)(*LINE), None if fill is None else (C.c_float * 3)(*fill),
            width, feather, opacity)
    winner = s.winner_without_gone if pos_of else s.winner
    kw = dict(width=width, line=LINE, feather=feather, opacity=opacity, fill=fill, edges=s.edges if masked else None, y0=y0, y1=y1)
    if outline:
        _capi.check(lib.crender_wire_outline(D.winner.data_ptr(), D.z.data_ptr(), *head, depth_bias, radius_px,
                                             color.data_ptr(), s.H, s.W, y0, y1, 0, stream()), "crender_wire_outline")
        key = (id(s), masked, pos_of, radius_px, depth_bias, y0, y1)
        if key not in _FIELDS:
            _FIELDS[key] = outline_ref.distances(winner, s.z, s.tri, E.P, kw["edges"], radius_px, depth_bias, y0, y1)
        want = outline_ref.wire_pass(s.color, winner, s.z, s.tri, E.P, depth_bias=depth_bias, radius_px=radius_px,
                                     field=_FIELDS[key], **kw)
    else:
        _capi.check(lib.crender_wire_overlay(D.winner.data_ptr(), *head, color.data_ptr(), s.H, s.W, y0, y1, 0, stream()),
                    "crender_wire_overlay")
        want = overlay_ref.wire_pass(s.color, winner, s.tri, E.P, **kw)
    assert not np.isnan(want).any()
    return color.cpu().numpy(), want


def _wire_every_variant(lib, D, what, outline, fill, masked, styles, **kw):
    """The whole frame under every style, then a strip of rows; what a pass without a fill may write is the covered
    pixels (the overlay) and the pixels on a line."""
    s = D.s
    covered = (s.winner >= 0) & (s.winner < s.T)
    changed = 0
    for style in styles:
        got, want = _wire(lib, D, outline, fill, masked, **style, **kw)
        assert_bit_equal(got, want, f"{what}, {style}")
        assert not np.isnan(got).any()
        moved = (want.view(np.uint32) != s.color.view(np.uint32)).any(2)
        changed += int(moved.sum())
        if not outline or kw.get("radius_px") == 0:
            assert not moved[~covered].any()
        if fill is not None:
            assert moved[covered].all()
    assert changed > (7844 if fill is not None else 40)
    y0, y1 = ROWS
    got, want = _wire(lib, D, outline, fill, masked, y0=y0, y1=y1, **styles[-1], **kw)
    assert_bit_equal(got[:y0], s.color[:y0], f"{what}: rows above the strip")
    assert_bit_equal(got[y1:], s.color[y1:], f"{what}: rows below the strip")
    assert_bit_equal(got, want, f"{what}, rows {y0} .. {y1}")
    D.untouched(what)                              # d_winner, d_z and d_tri among them


def _wire_pos_of(lib, D, what, outline, **kw):
    """The triangles moved, their corners fetched through d_pos_of and their edge bits where the caller put them."""
    s = D.s
    for fill in (None, FILL):
        got, want = _wire(lib, D, outline, fill, masked=True, pos_of=True, **kw)
        assert_bit_equal(got, want, f"{what}, d_pos_of, fill {fill}")
        gone = s.winner == s.gone
        if fill is None and not outline:
            assert_bit_equal(got[gone], s.color[gone], f"{what}: a triangle d_pos_of sends beyond T is background")
        other = _wire(lib, D, outline, fill, masked=True, **kw)[1]
        assert (want != other).any()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("fill", [None, FILL])
def test_wire_overlay_every_instance(lib, oracle, edge, fill, masked):
    what = f"overlay fill={fill} masked={masked}"
    styles = [dict(), dict(width=3.0, feather=0.5, opacity=0.5)] + ([WIDE] if fill is not None else [dict(WIDE, opacity=0.25)])
    _wire_every_variant(lib, edge, what, False, fill, masked, styles)
    if masked and fill is None:
        _wire_pos_of(lib, edge, what, False, width=3.0)


@pytest.mark.parametrize("radius_px", [0, 2, 8])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("fill", [None, FILL])
def test_wire_outline_every_instance(lib, oracle, edge, fill, masked, radius_px):
    """Windows that straddle the scene's 8 x 8 blocks of classes; corners at NaN and at infinity, edges of no length,
    a z plane with NaN and infinities, winners that name no triangle in the halo."""
    what = f"outline fill={fill} masked={masked} radius_px={radius_px}"
    styles = [dict(), dict(width=3.0, feather=0.5, opacity=0.5, depth_bias=0.0)] + \
             ([WIDE] if fill is not None else [dict(WIDE, opacity=0.25, depth_bias=-2e-3)])
    _wire_every_variant(lib, edge, what, True, fill, masked, styles, radius_px=radius_px)
    if masked and fill is None and radius_px == 2:
        _wire_pos_of(lib, edge, what, True, width=3.0, radius_px=3)


@pytest.fixture(scope="module")
def tie(oracle):
    return _Device(E.tie_scene())


@pytest.mark.parametrize("fill", [None, FILL])
def test_the_outline_at_the_tie_of_its_depth_test_and_on_every_side_of_its_clamp(lib, tie, fill):
    """The frame of tests/test_pass_edges_cpu.py's mutants: the kernel takes the edge one ulp above ze - depth_bias and
    at no other depth; its s is clamped at both ends; its ze is the depth at the closest point."""
    s = tie.s
    for style in (WIDE, dict(width=8.0, feather=2.0, opacity=0.5)):
        got, want = _wire(lib, tie, True, fill, masked=True, radius_px=E.TIE_RADIUS, depth_bias=E.TIE_BIAS, **style)
        assert_bit_equal(got, want, f"the tie frame, fill {fill}, {style}")
    got, want = _wire(lib, tie, True, fill, masked=True, radius_px=E.TIE_RADIUS, depth_bias=E.TIE_BIAS, **WIDE)
    lit = (got != s.color).any(2)
    assert lit[s.ring & (s.kind == 1)].all()
    if fill is None:                                   # (a fill stores every covered pixel)
        assert not lit[s.ring & (s.kind != 1)].any() and not lit[s.ring2 | s.is_a2].any()
    tie.untouched("the tie frame")


@pytest.fixture(scope="module")
def sparse(oracle):
    return {r: [_Device(s) for s in E.sparse_frames(r)] for r in E.SPARSE_RADII}


@pytest.mark.parametrize("radius_px", E.SPARSE_RADII)
def test_lone_winners_on_the_seams_of_the_outlines_tiles(lib, sparse, radius_px):
    """A frame of background but for lone winners, at most one in the rows any wavefront reaches: the wavefront may
    leave early only if that one is out of its reach, and the pixel exactly radius_px rows from it says whether it did
    (the model lights it: tests/test_pass_edges_cpu.py).  Every row residue in three tile rows, both signs, winners in
    the halo of the neighbouring tile, 97 x 101 pixels: the last tile row is one row, the last column five."""
    for k, D in enumerate(sparse[radius_px]):
        color = D.s.color
        for fill in (None, FILL):
            got, want = _wire(lib, D, True, fill, masked=True, radius_px=radius_px)
            assert_bit_equal(got, want, f"lone winners, radius {radius_px}, frame {k}, fill {fill}")
            nearer, want = _wire(lib, D, True, fill, masked=True, radius_px=radius_px - 1)
            assert_bit_equal(nearer, want, f"lone winners, radius {radius_px - 1}, frame {k}, fill {fill}")
            for t, x, y, px, py in E.extreme_taps(D.s, radius_px):
                assert (got[py, px] != color[py, px]).any() and (nearer[py, px] == color[py, px]).all(), (D.s.lone[t], px, py)
        D.untouched(f"lone winners, frame {k}")


@pytest.mark.parametrize("radius_px", E.SPARSE_RADII)
def test_the_outline_does_not_see_winners_outside_its_strip(lib, oracle, radius_px):
    D = _Device(E.sparse_strip())
    s = D.s
    y0, y1 = E.SPARSE_STRIP
    for fill in (None, FILL):
        got, want = _wire(lib, D, True, fill, masked=True, radius_px=radius_px, y0=y0, y1=y1)
        assert_bit_equal(got, want, f"the strip of lone winners, radius {radius_px}, fill {fill}")
        assert_bit_equal(got[:y0], s.color[:y0], "rows above the strip")
        assert_bit_equal(got[y1:], s.color[y1:], "rows below the strip")
        xc = s.lone[2][0]
        keep = np.ones(s.W, bool)
        keep[xc - radius_px:xc + radius_px + 1] = False
        assert_bit_equal(got[:, keep], s.color[:, keep], "the columns of the winners outside the strip")
        assert (got[y0:y1, xc] != s.color[y0:y1, xc]).any()
        whole = _wire(lib, D, True, fill, masked=True, radius_px=radius_px)[0]
        assert (whole[y0:y1][:, keep] != s.color[y0:y1][:, keep]).any()           # the whole frame does see them


# ---- the small frame: denominators under the window that are not zero ------------------------------------------------------

@pytest.mark.parametrize("kind,kw", [("tex", dict(persp=True, bilinear=True, light=False)), ("tex", dict(persp=False, bilinear=False, light=True)),
                                     ("mip", dict(persp=True, light=False)), ("mip", dict(persp=False, light=True)),
                                     ("aniso", dict(persp=True, A=16, light=True)), ("aniso", dict(persp=False, A=4, light=False)),
                                     ("phong", dict(lights="point", shininess=1)), ("phong", dict(lights="direction", shininess=4096)),
                                     ("phong", dict(lights="four", shininess=32)), ("ao", dict(radius_px=8)), ("ao", dict(radius_px=32)),
                                     ("wire", dict(width=1.0)), ("wire", dict(width=3.0, feather=0.5, opacity=0.5)),
                                     ("outline", dict(radius_px=8)), ("outline", dict(radius_px=8, width=9.0, feather=5.0, depth_bias=0.0)),
                                     ("outline", dict(radius_px=0, width=3.0))])
def test_the_small_frame(lib, oracle, mini, textures, kind, kw):
    if kind == "phong":
        got, want = _phong(lib, mini, mini.s.lights[kw["lights"]], kw["shininess"])
        assert np.isfinite(want).all()
        _same(got, want, f"28 x 20, phong {kw}")
    elif kind == "ao":               # the whole frame lies inside one tile and is smaller than the halo of 32
        table, radius = _ao_table(mini.s, kw["radius_px"])
        for face in (False, True):
            for rotate in (False, True):
                got, want = _ao(lib, mini, table, face, rotate, kw["radius_px"], radius)
                _same(got, want, f"28 x 20, ao face={face} rotate={rotate} {kw}")
    elif kind in ("wire", "outline"):                # 20 rows under a halo of 8: every tile row of the stage is partial
        for fill in (None, FILL):
            for masked in (False, True):
                got, want = _wire(lib, mini, kind == "outline", fill, masked, **kw)
                assert_bit_equal(got, want, f"28 x 20, {kind} {kw}, fill {fill}, masked {masked}")
                assert (want != mini.s.color).any()
    for name in ("64x97", "3x1000") if kind in ("tex", "mip", "aniso") else ():
        got, want = _texture_family(lib, oracle, mini, kind, textures[name], **kw)
        _same(got, want, f"28 x 20, {kind} {kw}, texture {name}")
    mini.untouched(f"28 x 20, {kind}")


def test_the_small_frame_shadowed(lib, oracle, mini):
    for K, use_winner in ((1, True), (3, False), (5, True)):
        got, want = _shadow(lib, mini, K, use_winner)
        _same(got, want, f"28 x 20, shadow K={K} use_winner={use_winner}")


# ---- the tall frame: the row-block loop's second trip --------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["tex", "mip", "aniso", "shadow", "phong", "wire", "outline"])
def test_more_row_blocks_than_the_grid_is_tall(lib, oracle, tall, textures, kind):
    """H = 524 296, W = 3, rows 3 .. H: 65 537 blocks of 8 rows against a grid of 65 535, so the last sixteen rows are
    the loop's second trip.  No plan can be that tall: only the entry reaches it.  The texture families run with the
    light, which touches every pixel of the rows; the Phong pass with four lights; the wire passes with a fill, which
    stores every covered pixel.  The outline has no such loop: it launches a workgroup per tile of 32 x 32, 16 385 of
    them, and is compared where anything can differ, as the model's walk over 1.5 M pixels is."""
    s = tall.s
    y0 = E.TALL_Y0
    if kind == "shadow":
        got, want = _shadow(lib, tall, 3, True, y0=y0)
    elif kind == "phong":
        got, want = _phong(lib, tall, s.lights["four"], y0=y0)
    elif kind in ("wire", "outline"):
        got, want = _wire(lib, tall, kind == "outline", FILL, masked=True, y0=y0, width=3.0, radius_px=2)
        assert_bit_equal(got[s.rows], want[s.rows], f"tall frame, {kind}: the rows that hold anything")
    else:
        kw = dict(tex=dict(persp=True, bilinear=True), mip=dict(persp=True), aniso=dict(persp=True, A=4))[kind]
        got, want = _texture_family(lib, oracle, tall, kind, textures["64x97"], light=True, y0=y0, **kw)
    assert_bit_equal(got[:y0], s.color[:y0], f"tall frame, {kind}: rows above y0")
    last = slice(E.TALL_H - 16, E.TALL_H)
    assert (want[last].view(np.uint32) != s.color[last].view(np.uint32)).any(), "the second trip's rows change"
    _same(got[last], want[last], f"tall frame, {kind}: the second trip's rows")
    _same(got, want, f"tall frame, {kind}")
