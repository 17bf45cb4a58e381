"""Mipmaps and trilinear filtering on the GPU (csrc/texmip.hip through bind_texture(..., mipmaps=True),
texture_pass(filter="trilinear") and Renderer(texture_pass=...)), bit for bit against the host model of
tests/mip_ref.py evaluated on the oracle's frame (itself pinned in tests/test_mipmap_cpu.py)."""
import numpy as np
import pytest

import mip_ref
import tex_ref
from pass_scenes import filler, host, oracle_frame, planes_only_read, soup_textured, texture, textured_model, trex_textured
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

LIGHT = (0.3, -0.2, 1.0)             # what GuroIllumination is constructed with
SIZES = [(1, 1), (1, 7), (2, 5), (3, 1000), (709, 709), (64, 97), (1025, 513)]


def _want(ref, tri, uv, tex, persp=False, **kw):
    return mip_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, perspective=persp, **kw)


def _levels(ref, tri, uv, tex, persp):
    return mip_ref.pixel_levels(ref.winner, tri, ref.proj_mat, uv, tex.shape[0], tex.shape[1], persp)[5]


def _check_both_modes(oracle, scene, tex, H, W, what, min_covered=1, check=None, **filler_kw):
    """The trilinear pass, affine and perspective, against the host model; `check(l0, L)` judges the levels."""
    tri, col, nrm, uv = scene
    ref = oracle_frame(oracle, tri, col, nrm, H, W)
    covered = int((ref.winner >= 0).sum())
    assert covered >= min_covered, (what, covered)
    f = filler(H, W, **filler_kw)
    f.bind_texture(uv, tex, mipmaps=True)
    chain = mip_ref.build_chain(tex)
    for persp in (False, True):
        f.render_arrays(tri, col, nrm, clear=True)
        f.texture_pass(perspective=persp, filter="trilinear")
        want = _want(ref, tri, uv, tex, persp, chain=chain)
        assert not np.isnan(want).any(), (what, persp)
        assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour, perspective={persp}")
        assert (want.view(np.uint32) != ref.color_buffer.view(np.uint32)).any(), (what, "the pass changed nothing")
        planes_only_read(f, ref, what)
        if check is not None:
            l0 = _levels(ref, tri, uv, tex, persp)
            print(f"{what}, perspective={persp}: levels {np.bincount(l0, minlength=len(chain)).tolist()}")
            check(l0, len(chain), want, ref, persp)
    return f


@pytest.mark.parametrize("th,tw", SIZES)
def test_chain_equals_the_host_model(th, tw):
    import torch
    tex = texture(th * 1000 + tw, th, tw)
    f = filler(16, 16)
    assert f.mip_levels() is None
    f.bind_texture(np.zeros((1, 3, 2), np.float32), tex, mipmaps=True)
    chain = mip_ref.build_chain(tex)
    assert f.mip_levels() == [c.shape[:2] for c in chain] == mip_ref.layout(th, tw)[0]
    for k, want in enumerate(chain):
        got = f.get_mip_level(k)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(host(got), want), f"{th} x {tw}, level {k}"
    assert np.array_equal(host(f._mip[0]), mip_ref.pack_chain(chain))          # packed tightly, in order
    assert f.get_mip_level(0).data_ptr() == f._mip[0].data_ptr()                # a view, not a copy
    uv, image = f._texture                                                      # still the (uv, image) pair
    assert np.array_equal(host(image), tex) and tuple(uv.shape) == (1, 3, 2)
    with pytest.raises(IndexError):
        f.get_mip_level(len(chain))


@pytest.mark.parametrize("size", [256, 1024])
def test_trex_against_the_host_model(oracle, size):
    tri, col, nrm, uv = trex_textured()
    tex = texture(1, 709, 709)

    def check(l0, L, want, ref, persp):
        bilinear = tex_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, perspective=persp,
                                        bilinear_filter=True)
        assert (bilinear.view(np.uint32) != want.view(np.uint32)).any()
        if size == 256:
            assert (l0 >= 1).sum() >= 5000 and (l0 == 0).sum() >= 100

    _check_both_modes(oracle, (tri, col, nrm, uv), tex, size, size, f"trex{size}", min_covered=15000, check=check)


@pytest.mark.parametrize("seed,T,H,W,th,tw", [(31, 4000, 200, 173, 1, 1), (32, 2500, 333, 512, 3, 1000),
                                              (33, 30000, 512, 509, 709, 709), (34, 60, 64, 41, 2, 5)])
def test_random_soups_with_uv_beyond_the_unit_square(oracle, seed, T, H, W, th, tw):
    scene = soup_textured(seed, T, max(H, W), size_px=(1.0, 60.0))

    def check(l0, L, want, ref, persp):
        assert L == len(mip_ref.layout(th, tw)[0])
        if seed == 31:
            assert L == 1 and not l0.any()                   # a 1 x 1 texture: pure level 0
        if seed in (32, 33):
            assert (l0 == L - 1).sum() >= 1000               # footprints beyond the whole texture clamp at the top
        if seed == 34:
            assert L == 3                                    # the tiny chain: 2 x 5, 1 x 2, 1 x 1

    _check_both_modes(oracle, scene, texture(seed, th, tw), H, W, f"soup{seed}", min_covered=H * W // 20, check=check)


def test_presort_gives_the_same_bits(oracle):
    scene = soup_textured(41, 20000, 512, size_px=(2.0, 30.0))
    f = _check_both_modes(oracle, scene, texture(41, 64, 97), 512, 512, "presorted soup", presort=True)
    assert f._order is not None          # the resident inputs are the tile-coherent copy: the pass went through pos_of


def test_fused_light_equals_the_pass_plus_the_illumination(oracle):
    tri, col, nrm, uv = trex_textured()
    tex = texture(5, 709, 709)
    chain = mip_ref.build_chain(tex)
    H = W = 512
    ref = oracle_frame(oracle, tri, col, nrm, H, W)
    light = [float(v) for v in oracle.guro_light(LIGHT)]
    f, g = filler(H, W), filler(H, W)
    f.bind_texture(uv, tex, mipmaps=True)
    g.bind_texture(uv, tex, mipmaps=True)
    for persp in (False, True):
        f.render_arrays(tri, col, nrm, clear=True)
        f.texture_pass(perspective=persp, filter="trilinear", light_direction=light)
        g.render_arrays(tri, col, nrm, clear=True)
        g.texture_pass(perspective=persp, filter="trilinear")
        g.synchronize()
        g.shade_guro(light)
        got = host(f.get_color_tensor())
        assert_bit_equal(got, host(g.get_color_tensor()), f"fused light vs pass + illumination, {persp}")
        want = _want(ref, tri, uv, tex, persp, chain=chain, normals=ref.normals_buffer, light_direction=LIGHT)
        assert_bit_equal(got, want, f"fused light vs oracle.guro of the host model, {persp}")
        assert_bit_equal(host(f.get_normals_tensor()), ref.normals_buffer, "normals")
    # the background is shaded too: a colour written there beforehand comes out multiplied
    f.render_arrays(tri, col, nrm, clear=True)
    plane = f.get_color_tensor()
    plane[0, 0, :] = 3.0
    nplane = f.get_normals_tensor()
    nplane[0, 0, 2] = -2.0
    f.texture_pass(filter="trilinear", light_direction=light)
    c = ref.color_buffer.copy(); c[0, 0, :] = 3.0
    n = ref.normals_buffer.copy(); n[0, 0, 2] = -2.0
    want = mip_ref.texture_pass(c, ref.winner, tri, ref.proj_mat, uv, tex, chain=chain, normals=n, light_direction=LIGHT)
    assert ref.winner[0, 0] < 0 and want[0, 0, 0] != 0.0 and want[0, 0, 0] != 3.0
    assert_bit_equal(host(f.get_color_tensor()), want, "background under the fused light")


def test_row_strip_leaves_the_other_rows_alone(oracle):
    tri, col, nrm, uv = trex_textured()
    tex = texture(6, 709, 709)
    chain = mip_ref.build_chain(tex)
    H = W = 512
    y0, y1 = 135, 301                    # not multiples of the kernel's 8-row blocks
    ref = oracle_frame(oracle, tri, col, nrm, H, W, y0=y0, y1=y1)
    light = [float(v) for v in oracle.guro_light(LIGHT)]
    for with_light in (False, True):
        f = filler(H, W, row_strip=(y0, y1))
        f.bind_texture(uv, tex, mipmaps=True)
        f.render_arrays(tri, col, nrm, clear=True)
        f.synchronize()
        # rows outside the strip: colours to be kept, and winners that WOULD be textured if the pass looked at them
        f.color_buffer[:y0] = 7.5
        f.color_buffer[y1:] = -2.25
        f.winner_buffer[:y0] = 0
        f.winner_buffer[y1:] = 1
        f.texture_pass(filter="trilinear", light_direction=light if with_light else None)
        got = host(f.get_color_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        kw = dict(normals=ref.normals_buffer, light_direction=LIGHT) if with_light else {}
        want = _want(ref, tri, uv, tex, False, chain=chain, y0=y0, y1=y1, **kw)
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, light={with_light}")


def test_nan_and_infinite_uv_follow_the_statement(oracle):
    tri, col, nrm, uv = soup_textured(12, 1500, 160, size_px=(4.0, 40.0))
    rng = np.random.default_rng(12)
    odd = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 2147483648.0, -2147483904.0, 1e-42])
    hit = rng.uniform(size=uv.shape) < 0.15
    uv[hit] = rng.choice(odd, int(hit.sum()))
    tex = texture(12, 5, 7)
    ref = oracle_frame(oracle, tri, col, nrm, 160, 160)
    f = filler(160, 160)
    f.bind_texture(uv, tex, mipmaps=True)
    for persp in (False, True):
        f.render_arrays(tri, col, nrm, clear=True)
        f.texture_pass(perspective=persp, filter="trilinear")
        got = host(f.get_color_tensor())
        want = _want(ref, tri, uv, tex, persp)
        # (IEEE 754 leaves the sign and payload of a generated NaN open: x86 and gfx950 differ there)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), persp
        assert_bit_equal(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), f"odd uv, {persp}")
        assert nan.any() and not nan.all()


@pytest.mark.parametrize("on_device", [None, False, True, "fused"])
def test_renderer_under_every_on_device(oracle, on_device):
    from cython3dmodelrenderer_amd.illumination.guro_illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    m, tex = textured_model()
    tri, col, nrm = m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles
    uv = m.get_texture_coords_by_triangles()
    H = W = 256
    ref = oracle_frame(oracle, tri, col, nrm, H, W)
    assert int((ref.winner >= 0).sum()) > 10000
    want = _want(ref, tri, uv, tex, True, normals=ref.normals_buffer, light_direction=LIGHT)
    bilinear = tex_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, perspective=True,
                                    bilinear_filter=True, normals=ref.normals_buffer, light_direction=LIGHT)
    assert (want != bilinear).any()
    f = filler(H, W)
    binds = []
    bind = f.bind_texture
    f.bind_texture = lambda *a, **kw: (binds.append(kw), bind(*a, **kw))[1]
    r = Renderer(f, GuroIllumination(LIGHT), on_device=on_device, texture_pass={"filter": "trilinear", "perspective": True})
    for _ in range(2):                             # every frame starts from cleared buffers: the same image twice
        out = r.render(m)
        got = host(out) if on_device in (True, "fused") else np.array(out)
        assert_bit_equal(got, want, f"Renderer(on_device={on_device!r})")
    assert binds == [{"mipmaps": True}]            # the texture went up once per model, with its chain
    assert f.mip_levels() == mip_ref.layout(37, 53)[0]
    assert_bit_equal(host(f.get_normals_tensor()), ref.normals_buffer, "normals")


def test_errors_name_their_cause(oracle):
    from cython3dmodelrenderer_amd import _capi
    tri, col, nrm, uv = soup_textured(13, 300, 64)
    tex = texture(13, 8, 8)
    f = filler(64, 64)
    f.bind_texture(uv, tex, mipmaps=True)
    assert f.mip_levels() == [(8, 8), (4, 4), (2, 2), (1, 1)]
    f.render_arrays(tri, col, nrm, clear=True)
    f.texture_pass(filter="trilinear")
    # an error of the entry point surfaces with its name: a flag it does not know, refused before any launch
    d_uv, _ = f._texture
    rc = f._lib.crender_mip_shade(f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), len(tri), None, f._P,
                                  d_uv.data_ptr(), f._mip[0].data_ptr(), 8, 8, None, None, f.color_buffer.data_ptr(),
                                  64, 64, 0, 64, _capi.TEX_BILINEAR, f._stream())
    assert rc == _capi.EINVAL
    with pytest.raises(_capi.CrenderError, match="crender_mip_shade failed.*crender_mip_shade: bad argument"):
        _capi.check(rc, "crender_mip_shade")
    # rebinding without the chain drops it: trilinear names its filter, bilinear goes on working
    f.bind_texture(uv, tex)
    assert f.mip_levels() is None
    with pytest.raises(ValueError, match="filter 'trilinear' needs a mip chain"):
        f.texture_pass(filter="trilinear")
    with pytest.raises(ValueError):
        f.get_mip_level(0)
    f.texture_pass(filter="bilinear")
    f.bind_texture(uv, tex, mipmaps=True)
    f.bind_texture(None, None)
    assert f.mip_levels() is None and f._texture is None
    with pytest.raises(ValueError, match="no texture is bound"):
        f.texture_pass(filter="trilinear")
    with pytest.raises(ValueError, match="filter"):
        f.texture_pass(filter="anisotropic")
    chain = filler(64, 64, pipeline=True)
    chain.bind_texture(uv, tex, mipmaps=True)
    with pytest.raises(ValueError, match="swap chain"):
        chain.texture_pass(filter="trilinear")
