"""The supersampling resolve on the GPU (csrc/resolve.hip through crender_ssaa_resolve, ``DevicePlanes.resolve`` and
``Renderer(supersample=...)``), bit for bit against the host model of tests/ssaa_ref.py (itself pinned by hand in
tests/test_ssaa_cpu.py).  (The fused-light case renders its soup at 64 x 48 for s = 2 and at 63 x 48 for s = 3:
64 is no multiple of 3.)"""
import ctypes as C
import os

import numpy as np
import pytest

import ssaa_ref
from pass_scenes import GOLDEN, filler, host, lib, light3, stream, trex_arrays  # noqa: F401 (lib is a fixture)
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

LIGHT = (0.3, -0.2, 1.0)             # what GuroIllumination is constructed with
# Ho x Wo: Wo no multiple of 64 and Wo * 3 no multiple of 4; the second crosses a wavefront, the third a workgroup
SIZES = ((23, 41), (7, 130), (3, 301))


def _device(a, offset=0):
    """`a` on the device, `offset` floats past an aligned address (-> the tensor, kept alive by the caller)."""
    import torch
    flat = torch.empty(a.size + offset, dtype=torch.float32, device="cuda:0")
    view = flat[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _resolve(lib, color, normals, light, s, Y0, Y1, out, flags):
    from cython3dmodelrenderer_amd import _capi
    H, W = color.shape[:2]
    _capi.check(lib.crender_ssaa_resolve(color.data_ptr(), None if normals is None else normals.data_ptr(), light,
                                         H, W, s, Y0, Y1, out.data_ptr(), flags, stream()), "crender_ssaa_resolve")


def _random_planes(seed, H, W):
    rng = np.random.default_rng(seed)
    color = rng.uniform(-300, 300, (H, W, 3)).astype(np.float32)
    normals = rng.standard_normal((H, W, 3)).astype(np.float32)
    normals[rng.uniform(size=H) < 0.3] = 0.0          # rows of background: the factor of a zero normal
    normals[0, 0] = 0.0
    return color, normals


class _M:
    def __init__(self, tri, col, nrm=None, uv=None, tex=None):
        self._vertices_by_triangles, self._colors_by_triangles, self._normals_by_triangles = tri, col, nrm
        self._uv, self._tex = uv, tex

    def get_texture_coords_by_triangles(self):
        return self._uv

    def get_texture(self):
        return self._tex


# ---- random planes through every kernel instance ---------------------------------------------------------------

@pytest.mark.parametrize("s", range(1, 9))
def test_random_planes_every_instance(lib, oracle, s):
    import torch
    from cython3dmodelrenderer_amd import _capi
    light = light3(oracle)
    # the wide loads of an even factor are as aligned as the planes: also 1 and 2 floats past an aligned address
    offsets = (0,) if s % 2 else ((0, 1) if s % 4 else (0, 1, 2))
    for Ho, Wo in SIZES:
        color, normals = _random_planes(100 * s + Wo, Ho * s, Wo * s)
        for with_light in (False, True):
            want = ssaa_ref.resolve(color, s, normals=normals, light_direction=LIGHT if with_light else None)
            assert want.shape == (Ho, Wo, 3) and not np.isnan(want).any()
            if s > 1:
                assert (want != color[::s, ::s]).any()
            want_u8 = ssaa_ref.present_u8(want)
            assert want.min() < -1 and want.max() > 1       # the cast sees both signs
            for offset in offsets:
                d_color, d_normals = _device(color, offset), _device(normals, offset)
                assert d_color.data_ptr() % 16 == 4 * offset
                for flags in range(4):
                    u8, flip = bool(flags & _capi.SSAA_U8), bool(flags & _capi.SSAA_FLIP)
                    out = torch.full((Ho, Wo, 3), 77, dtype=torch.uint8 if u8 else torch.float32, device="cuda:0")
                    _resolve(lib, d_color, d_normals if with_light else None, light if with_light else None, s, 0, Ho,
                             out, flags)
                    ref = want_u8 if u8 else want
                    assert_bit_equal(host(out), ref[::-1] if flip else ref,
                                     f"s={s} {Ho}x{Wo} light={with_light} u8={u8} flip={flip} offset={offset}")
                # the source planes are only read
                assert_bit_equal(host(d_color), color, "source colour")
                assert_bit_equal(host(d_normals), normals, "source normals")


# ---- special values by hand --------------------------------------------------------------------------------------

def test_special_values(lib):
    import torch
    from cython3dmodelrenderer_amd import _capi
    nan, inf = np.nan, np.inf
    blocks = [[nan, 1, 2, 3], [1, 2, 3, nan], [inf, 1, 1, 1], [-inf, inf, 0, 0], [-0.0, -0.0, -0.0, -0.0],
              [0.0, -0.0, -0.0, -0.0], [1e-45, 1e-45, 1e-45, 0], [1e-39, 2e-39, -1e-39, 3e-42], [3e38, 3e38, 1, 1],
              [3e38, -3e38, 3e38, -3e38], [-3e38, -3e38, -3e38, 5], [1e8, 1, -1e8, 1], [255.9, 255.9, 255.9, 255.9],
              [-1.5, -1.5, -1.5, -1.5], [4e10, 1, 1, 1], [1.1754944e-38, 0, 0, 0]]
    src = np.zeros((8, 8, 3), np.float32)                 # 4 x 4 blocks of 2 x 2
    for k, b in enumerate(blocks):
        Y, X = divmod(k, 4)
        src[2 * Y:2 * Y + 2, 2 * X:2 * X + 2] = np.float32(b).reshape(2, 2, 1) * np.float32([1, -1, 0.5])
    d_src = _device(src)
    for s in (1, 2, 4):
        want = ssaa_ref.resolve(src, s)
        where = np.isnan(want)
        assert where.any() and not where.all()
        if s == 2:
            assert where[0, 0].all() and where[0, 1].all() and where[0, 3].all() and not where[0, 2].any()
            assert np.isinf(want[2, 0, 0]) and want[2, 1, 0] == 0 and np.signbit(want[1, 0, 0])
            assert not np.signbit(want[1, 1, 0]) and 0 < want[1, 2, 0] < 1e-44      # +0 + -0; a denormal mean
        for flip in (0, _capi.SSAA_FLIP):
            out = torch.zeros(want.shape, dtype=torch.float32, device="cuda:0")
            _resolve(lib, d_src, None, None, s, 0, 8 // s, out, flip)
            got = host(out)[::-1] if flip else host(out)
            # (IEEE 754 leaves the sign and payload of a generated NaN open: x86 and gfx950 differ there)
            assert np.array_equal(np.isnan(got), where), s
            assert_bit_equal(np.where(where, np.float32(0), got), np.where(where, np.float32(0), want), f"float32, s={s}")
            out8 = torch.full(want.shape, 9, dtype=torch.uint8, device="cuda:0")
            _resolve(lib, d_src, None, None, s, 0, 8 // s, out8, flip | _capi.SSAA_U8)
            got8 = host(out8)[::-1] if flip else host(out8)
            assert_bit_equal(got8, ssaa_ref.present_u8(want), f"uint8, s={s}")


# ---- the three identities of s = 1 -------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(37, 53), (70001, 3)])         # the second: more rows than the grid is tall
def test_a_factor_of_one_is_the_copy_the_illumination_and_the_presentation(lib, oracle, H, W):
    import torch
    from cython3dmodelrenderer_amd import _capi
    color, normals = _random_planes(H, H, W)
    color[1, 2] = [-0.0, 0.0, -0.0]
    d_color, d_normals = _device(color), _device(normals)
    light = light3(oracle)
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    _resolve(lib, d_color, None, None, 1, 0, H, out, 0)
    assert_bit_equal(host(out), color, "s = 1: the plane itself")
    # with a light: crender_guro_illumination on a copy
    shaded = d_color.clone()
    _capi.check(lib.crender_guro_illumination(shaded.data_ptr(), d_normals.data_ptr(), light, H, W, 0, H, stream()),
                "crender_guro_illumination")
    _resolve(lib, d_color, d_normals, light, 1, 0, H, out, 0)
    assert_bit_equal(host(out), host(shaded), "s = 1 with a light: the illumination pass")
    assert_bit_equal(host(out), ssaa_ref.shade(color, normals, LIGHT), "and the oracle's statements")
    assert (host(out) != color).any()
    # with U8 (| FLIP): crender_present_u8
    for flip in (0, 1):
        want = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda:0")
        _capi.check(lib.crender_present_u8(d_color.data_ptr(), want.data_ptr(), H, W, flip, stream()), "crender_present_u8")
        out8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda:0")
        _resolve(lib, d_color, None, None, 1, 0, H, out8, _capi.SSAA_U8 | (_capi.SSAA_FLIP if flip else 0))
        assert_bit_equal(host(out8), host(want), f"s = 1, uint8, flip={flip}: the presentation")
        assert_bit_equal(host(out8), ssaa_ref.present_u8(color, flip_rows=bool(flip)), "and the model's cast")


# ---- the fused light is the pass plus the resolve ---------------------------------------------------------------

@pytest.mark.parametrize("s,W", [(2, 64), (3, 63)])
def test_fused_light_equals_the_illumination_pass_plus_the_resolve(oracle, s, W):
    H = 48
    tri, col, nrm = random_soup(np.random.default_rng(7), 60, 64, size_px=(4.0, 40.0))
    ref = oracle.OracleFiller(H, W, fov=45.0)
    ref.render_arrays(tri, col, nrm)
    assert int((ref.normals_buffer != 0).any(axis=2).sum()) > 300
    light = [float(v) for v in oracle.guro_light(LIGHT)]
    f, g = filler(H, W), filler(H, W)
    f.render_arrays(tri, col, nrm, clear=True)
    g.render_arrays(tri, col, nrm, clear=True)
    fused = host(f.resolve(s, light_direction=light))
    assert_bit_equal(host(f.get_color_tensor()), ref.color_buffer, "the source colour stays unshaded")
    g.synchronize()
    g.shade_guro(light)
    assert_bit_equal(fused, host(g.resolve(s)), f"s={s}: fused light vs shade_guro + plain resolve")
    want = ssaa_ref.resolve(ref.color_buffer, s, normals=ref.normals_buffer, light_direction=LIGHT)
    assert not np.isnan(want).any() and (want != ssaa_ref.resolve(ref.color_buffer, s)).any()
    assert_bit_equal(fused, want, f"s={s}: fused light vs the model")
    assert_bit_equal(host(f.resolve(s, light_direction=light, dtype="uint8", flip_rows=True)),
                     ssaa_ref.present_u8(want, flip_rows=True), f"s={s}: fused light, uint8, flipped")


# ---- rows --------------------------------------------------------------------------------------------------------

def test_rows_through_the_entry_point_keep_a_sentinel(lib, oracle):
    import torch
    from cython3dmodelrenderer_amd import _capi
    s, Ho, Wo = 3, 11, 70
    color, normals = _random_planes(11, Ho * s, Wo * s)
    d_color, d_normals = _device(color), _device(normals)
    light = light3(oracle)
    want = ssaa_ref.resolve(color, s, normals=normals, light_direction=LIGHT)
    for Y0, Y1 in ((2, 9), (4, 5), (0, 1), (10, 11)):
        for flags in range(4):
            u8, flip = bool(flags & _capi.SSAA_U8), bool(flags & _capi.SSAA_FLIP)
            out = torch.full((Ho, Wo, 3), 77, dtype=torch.uint8 if u8 else torch.float32, device="cuda:0")
            _resolve(lib, d_color, d_normals, light, s, Y0, Y1, out, flags)
            ref = np.full((Ho, Wo, 3), 77, np.uint8 if u8 else np.float32)
            ssaa_ref.resolve(color, s, normals=normals, light_direction=LIGHT, dtype="uint8" if u8 else "float32",
                             flip_rows=flip, Y0=Y0, Y1=Y1, out=ref)
            assert (ref == 77).all(axis=(1, 2)).sum() == Ho - (Y1 - Y0)
            assert_bit_equal(host(out), ref, f"rows {Y0}..{Y1}, u8={u8}, flip={flip}")
    assert_bit_equal(ssaa_ref.resolve(color, s, normals=normals, light_direction=LIGHT, Y0=2, Y1=9)[2:9], want[2:9], "model")


def test_a_row_strip_filler_resolves_its_rows(oracle):
    H, W, s = 96, 80, 4
    y0, y1 = 24, 68
    tri, col, nrm = random_soup(np.random.default_rng(9), 200, 96, size_px=(4.0, 40.0))
    ref = oracle.OracleFiller(H, W, fov=45.0)
    ref.render_arrays(tri, col, nrm, y0=y0, y1=y1)
    f = filler(H, W, row_strip=(y0, y1))
    f.render_arrays(tri, col, nrm, clear=True)
    f.synchronize()
    f.color_buffer[:y0] = 7.5            # rows outside the strip are not the filler's: never read
    f.color_buffer[y1:] = -2.25
    got = host(f.resolve(s))
    want = ssaa_ref.resolve(ref.color_buffer, s)
    assert got.shape == (24, 20, 3)
    assert_bit_equal(got[6:17], want[6:17], "the strip's rows")
    assert (want[6:17] != 0).any() and not got[:6].any() and not got[17:].any()
    got8 = host(f.resolve(s, dtype="uint8", flip_rows=True))
    assert_bit_equal(got8[24 - 17:24 - 6], ssaa_ref.present_u8(want[6:17], flip_rows=True), "flipped strip")
    assert not got8[:24 - 17].any() and not got8[24 - 6:].any()
    assert_bit_equal(host(f.resolve(2))[12:34], ssaa_ref.resolve(ref.color_buffer, 2)[12:34], "s = 2")
    for bad in (8, 3):                   # 96 x 80 is a multiple of 8; 24 .. 68 is not.  68 is no multiple of 3
        with pytest.raises(ValueError, match="multiple"):
            f.resolve(bad)
    g = filler(H, W, row_strip=(24, 66))
    g.render_arrays(tri, col, nrm, clear=True)
    with pytest.raises(ValueError, match=r"row strip \(24, 66\).*factor=4"):
        g.resolve(4)


# ---- end to end --------------------------------------------------------------------------------------------------

def _numpy(image):
    import torch
    return host(image) if isinstance(image, torch.Tensor) else np.array(image)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("on_device", [None, False, True, "fused"])
def test_renderer_supersample_under_every_on_device(on_device, s):
    import torch
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    size = 256
    model = _M(*trex_arrays())
    plain = Renderer(filler(size, size), GuroIllumination(LIGHT), None, size, size, on_device=on_device)
    full = _numpy(plain.render(model))
    want = ssaa_ref.resolve(full, s)
    assert not np.isnan(want).any() and (want != full[::s, ::s]).any()
    f = filler(size, size)
    r = Renderer(f, GuroIllumination(LIGHT), None, size, size, on_device=on_device, supersample=s)
    for _ in range(2 if on_device == "fused" else 1):          # (the other modes composite: the same frame anyway)
        out = r.render(model)
        assert isinstance(out, torch.Tensor if on_device in (True, "fused") else np.ndarray)
        assert tuple(out.shape) == (size // s, size // s, 3)
        assert_bit_equal(_numpy(out), want, f"Renderer(on_device={on_device!r}, supersample={s})")
    shaded = on_device in (False, "fused")
    unshaded = filler(size, size)
    unshaded.render_model(model, clear=True)
    same = np.array_equal(host(f.get_color_tensor()), host(unshaded.get_color_tensor()))
    assert same != shaded                # the resolve carried the light: the filler's colour plane stays unshaded
    if not isinstance(out, torch.Tensor):
        assert not any(np.shares_memory(out, v) for v in f._host.values())     # a copy, not a live view
    # the PNG's bytes, the documented way
    if not shaded:
        png = f.resolve(s, light_direction=GuroIllumination(LIGHT).light_direction, dtype="uint8", flip_rows=True)
        assert_bit_equal(host(png), ssaa_ref.present_u8(want, flip_rows=True), "uint8, flipped")


@pytest.mark.parametrize("s", [2, 4])
def test_renderer_supersample_with_the_texture_pass(s):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    size = 256
    with np.load(os.path.join(GOLDEN, "trex_uv.npz")) as z:
        uv = np.ascontiguousarray(z["uv"][z["faces_uv"]], dtype=np.float32)
    tex = np.random.default_rng(1).integers(0, 256, (709, 709, 3), dtype=np.uint8)
    model = _M(*trex_arrays(), uv=uv, tex=tex)
    tp = {"perspective": True, "filter": "trilinear", "anisotropy": 4}
    plain = Renderer(filler(size, size), GuroIllumination(LIGHT), None, size, size, on_device="fused", texture_pass=tp)
    full = _numpy(plain.render(model))
    untextured = _numpy(Renderer(filler(size, size), GuroIllumination(LIGHT), None, size, size,
                                 on_device="fused").render(model))
    assert (full != untextured).any()
    want = ssaa_ref.resolve(full, s)
    assert not np.isnan(want).any()
    r = Renderer(filler(size, size), GuroIllumination(LIGHT), None, size, size, on_device="fused", texture_pass=tp,
                 supersample=s)
    assert_bit_equal(_numpy(r.render(model)), want, f"textured, supersample={s}")


def test_the_wireframe_filler_resolves_too():
    from cython3dmodelrenderer_amd import scenes
    from cython3dmodelrenderer_amd.illumination.illumination_drawer import NoIllumination
    from cython3dmodelrenderer_amd.pixel_buffer_filler import EdgeOnlyPixelBufferFiller, LineBresenham
    from cython3dmodelrenderer_amd.renderer import Renderer
    size = 256
    tri, col, _ = trex_arrays()
    model = _M(scenes.fit_soup_to_frame(tri, size, size), col)

    def wire():
        return EdgeOnlyPixelBufferFiller(LineBresenham(), (255.0, 128.0, 3.0), h=size, w=size, device="cuda:0")

    plain = wire()
    plain.render_model(model)
    full = host(plain.get_color_tensor())
    assert 0 < (full != 0).any(axis=2).mean() < 1
    for s in (2, 4):
        want = ssaa_ref.resolve(full, s)
        levels = np.unique(want[:, :, 0])
        assert len(levels) > 2           # edges come out in shades between the background and the line colour
        for on_device in (None, False, True, "fused"):
            f = wire()
            out = Renderer(f, NoIllumination(), None, size, size, on_device=on_device, supersample=s).render(model)
            assert_bit_equal(_numpy(out), want, f"wireframe, on_device={on_device!r}, supersample={s}")
        assert_bit_equal(host(f.resolve(s, dtype="uint8", flip_rows=True)), ssaa_ref.present_u8(want, flip_rows=True),
                         f"wireframe uint8, s={s}")


# ---- a swap chain --------------------------------------------------------------------------------------------------

def test_resolve_after_pipelined_frames(oracle):
    size = 256
    tri, col, nrm = trex_arrays()
    f = filler(size, size, pipeline=True)
    f.render_arrays(tri, col, nrm, clear=True)
    for _ in range(3):
        f.render_frame()
    got = host(f.resolve(2))
    color = host(f.get_color_tensor())
    assert (color != 0).any()
    assert_bit_equal(got, ssaa_ref.resolve(color, 2), "the most recently submitted frame, resolved")
    light = [float(v) for v in oracle.guro_light(LIGHT)]
    for _ in range(2):
        f.render_frame()
    lit = host(f.resolve(4, light_direction=light))
    want = ssaa_ref.resolve(host(f.get_color_tensor()), 4, normals=host(f.get_normals_tensor()), light_direction=LIGHT)
    assert_bit_equal(lit, want, "with the light, after two more frames")


# ---- errors --------------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(lib):
    import torch
    from cython3dmodelrenderer_amd import _capi
    tri, col, nrm = random_soup(np.random.default_rng(13), 50, 64)
    f = filler(60, 64)
    f.render_arrays(tri, col, nrm, clear=True)
    assert tuple(f.resolve(4).shape) == (15, 16, 3)
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="factor must be an int from 1 to 8"):
            f.resolve(bad)
    with pytest.raises(ValueError, match="60 x 64 is not a multiple of factor=8"):
        f.resolve(8)
    with pytest.raises(ValueError, match="dtype must be 'float32' or 'uint8'"):
        f.resolve(2, dtype="float16")
    # an error of the entry point surfaces with its text: a light without normals, before any launch
    out = torch.zeros((30, 32, 3), dtype=torch.float32, device="cuda:0")
    light = (C.c_float * 3)(0, 0, -1)
    rc = lib.crender_ssaa_resolve(f.color_buffer.data_ptr(), None, light, 60, 64, 2, 0, 30, out.data_ptr(), 0, stream())
    assert rc == _capi.EINVAL
    with pytest.raises(_capi.CrenderError, match="crender_ssaa_resolve failed.*a light without normals"):
        _capi.check(rc, "crender_ssaa_resolve")
    rc = lib.crender_ssaa_resolve(f.color_buffer.data_ptr(), None, None, 60, 64, 7, 0, 8, out.data_ptr(), 0, stream())
    assert rc == _capi.EINVAL and b"multiple of s" in lib.crender_last_error()
    torch.cuda.synchronize()
    assert not host(out).any()
