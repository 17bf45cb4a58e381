"""Anisotropic filtering on the GPU (csrc/texaniso.hip through texture_pass(filter="trilinear", anisotropy=A) and
Renderer(texture_pass=...)), bit for bit against the host model of tests/aniso_ref.py evaluated on the oracle's
frame (itself pinned in tests/test_aniso_cpu.py)."""
import numpy as np
import pytest

import aniso_ref
import mip_ref
from pass_scenes import filler, host, oracle_frame, planes_only_read, soup_textured, texture, textured_model, trex_textured
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

LIGHT = (0.3, -0.2, 1.0)             # what GuroIllumination is constructed with


def _want(ref, tri, uv, tex, persp, A, **kw):
    return aniso_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, persp, A, **kw)


def _counts(ref, tri, uv, tex, persp, A):
    """Pixels per sample count: [0, #N=1, ..., #N=16]."""
    N = aniso_ref.pixel_footprints(ref.winner, tri, ref.proj_mat, uv, tex.shape[0], tex.shape[1], persp, A)[6]
    return np.bincount(N, minlength=17)


def _check_both_modes(oracle, scene, tex, H, W, what, levels, check=None, **filler_kw):
    """The pass at each A of `levels`, affine and perspective, against the host model; `check(counts, persp, A)`
    judges the sample counts."""
    tri, col, nrm, uv = scene
    ref = oracle_frame(oracle, tri, col, nrm, H, W)
    f = filler(H, W, **filler_kw)
    f.bind_texture(uv, tex, mipmaps=True)
    chain = mip_ref.build_chain(tex)
    constant = (chain[0] == chain[0][0, 0]).all()      # (a 1 x 1 texture: every filter gives its one texel)
    for persp in (False, True):
        trilinear = mip_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, persp, chain=chain)
        for A in levels:
            f.render_arrays(tri, col, nrm, clear=True)
            f.texture_pass(perspective=persp, filter="trilinear", anisotropy=A)
            want = _want(ref, tri, uv, tex, persp, A, chain=chain)
            assert not np.isnan(want).any(), (what, persp, A)
            assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour, perspective={persp}, A={A}")
            if not constant:
                assert (want.view(np.uint32) != trilinear.view(np.uint32)).any(), (what, A, "no pixel differs from trilinear")
            planes_only_read(f, ref, what)
            counts = _counts(ref, tri, uv, tex, persp, A)
            print(f"{what}, perspective={persp}, A={A}: {int(counts.sum())} covered, N histogram {counts[1:].tolist()}")
            if check is not None:
                check(counts, persp, A)
    return f


def test_the_floor_reaches_every_sample_count(oracle):
    def check(counts, persp, A):
        assert counts.sum() == 1968 and not counts[A + 1:].any()
        if persp and A == 16:
            assert (counts[1:] > 0).all() and counts[16] >= 100, counts.tolist()
        if persp:
            assert counts[1] >= 500                  # the near rows are magnified: the plain trilinear path

    _check_both_modes(oracle, aniso_ref.floor_scene(), texture(1, 256, 256), 64, 64, "floor64", (2, 4, 5, 16), check)


@pytest.mark.parametrize("size", [256, 1024])
def test_trex_against_the_host_model(oracle, size):
    def check(counts, persp, A):
        if size == 256:
            assert counts.sum() == 15801 and counts[1] == 0          # every covered pixel takes the sample loop
        elif A == 16 and not persp:
            # a wavefront mixes lanes that take one sample with lanes that take up to sixteen
            assert counts[1] >= 100000 and counts[2:].sum() >= 50000 and counts[16] >= 1

    _check_both_modes(oracle, trex_textured(), texture(1, 709, 709), size, size, f"trex{size}", (4, 16), check)


@pytest.mark.parametrize("seed,T,H,W,th,tw,size_px", [(34, 60, 64, 41, 2, 5, (1.0, 60.0)),
                                                      (31, 4000, 200, 173, 1, 1, (1.0, 60.0)),
                                                      (32, 2500, 333, 512, 3, 1000, (1.0, 60.0)),
                                                      (35, 1500, 128, 119, 64, 97, (2, 40))])
def test_random_soups_with_uv_beyond_the_unit_square(oracle, seed, T, H, W, th, tw, size_px):
    scene = soup_textured(seed, T, max(H, W), size_px=size_px)

    def check(counts, persp, A):
        if seed == 32:
            assert counts.sum() == 137178
            if A == 16 and not persp:
                assert counts[16] >= 10000           # clamped at the sample count
        if seed == 34:
            assert counts.sum() == 1886 and counts[2:5].sum() >= 100 and not counts[5:].any()

    _check_both_modes(oracle, scene, texture(seed, th, tw), H, W, f"soup{seed}", (3, 5, 16), check)


def test_nan_and_infinite_uv_follow_the_statement(oracle):
    tri, col, nrm, uv = soup_textured(12, 1500, 160, size_px=(4.0, 40.0))
    rng = np.random.default_rng(12)
    odd = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 2147483648.0, -2147483904.0, 1e-42])
    hit = rng.uniform(size=uv.shape) < 0.15
    uv[hit] = rng.choice(odd, int(hit.sum()))
    tex = texture(12, 5, 7)
    ref = oracle_frame(oracle, tri, col, nrm, 160, 160)
    assert int((ref.winner >= 0).sum()) == 25325
    f = filler(160, 160)
    f.bind_texture(uv, tex, mipmaps=True)
    for persp in (False, True):
        trilinear = mip_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, persp)
        for A in (5, 16):
            f.render_arrays(tri, col, nrm, clear=True)
            f.texture_pass(perspective=persp, filter="trilinear", anisotropy=A)
            got = host(f.get_color_tensor())
            want = _want(ref, tri, uv, tex, persp, A)
            # (IEEE 754 leaves the sign and payload of a generated NaN open: x86 and gfx950 differ there)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (persp, A)
            assert_bit_equal(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), f"odd uv, {persp}, {A}")
            assert nan.any() and not nan.all()
            # the pixels that are NaN are trilinear's: a lane with N == 1 never multiplies an infinite step by 0
            assert np.array_equal(nan, np.isnan(trilinear)), (persp, A)
            if not persp:
                assert int(nan.all(axis=2).sum()) == 6194


def test_one_sample_through_the_entry_point_is_the_trilinear_pass(oracle):
    from cython3dmodelrenderer_amd import _capi
    tri, col, nrm, uv = trex_textured()
    tex = texture(1, 709, 709)
    f, g = filler(256, 256), filler(256, 256)
    for x in (f, g):
        x.bind_texture(uv, tex, mipmaps=True)
    for persp in (False, True):
        f.render_arrays(tri, col, nrm, clear=True)
        f.texture_pass(perspective=persp, filter="trilinear")
        g.render_arrays(tri, col, nrm, clear=True)
        g.synchronize()
        before = host(g.get_color_tensor()).copy()
        d_uv, _ = g._texture
        _capi.check(g._lib.crender_aniso_shade(
            g.winner_buffer.data_ptr(), g._inputs[0].data_ptr(), len(tri), None, g._P, d_uv.data_ptr(),
            g._mip[0].data_ptr(), 709, 709, None, None, g.color_buffer.data_ptr(), 256, 256, 0, 256,
            _capi.MIP_PERSPECTIVE if persp else 0, 1, g._stream()), "crender_aniso_shade")
        g.synchronize()
        got = host(g.color_buffer)
        assert (got != before).any()
        assert_bit_equal(got, host(f.get_color_tensor()), f"max_aniso = 1 vs crender_mip_shade, perspective={persp}")


def test_presort_gives_the_same_bits(oracle):
    scene = soup_textured(41, 20000, 512, size_px=(2.0, 30.0))
    f = _check_both_modes(oracle, scene, texture(41, 64, 97), 512, 512, "presorted soup", (16,), presort=True)
    assert f._order is not None          # the resident inputs are the tile-coherent copy: the pass went through pos_of


def test_fused_light_equals_the_pass_plus_the_illumination(oracle):
    tri, col, nrm, uv = trex_textured()
    tex = texture(5, 709, 709)
    chain = mip_ref.build_chain(tex)
    H = W = 512
    A = 16
    ref = oracle_frame(oracle, tri, col, nrm, H, W)
    light = [float(v) for v in oracle.guro_light(LIGHT)]
    f, g = filler(H, W), filler(H, W)
    f.bind_texture(uv, tex, mipmaps=True)
    g.bind_texture(uv, tex, mipmaps=True)
    for persp in (False, True):
        f.render_arrays(tri, col, nrm, clear=True)
        f.texture_pass(perspective=persp, filter="trilinear", light_direction=light, anisotropy=A)
        g.render_arrays(tri, col, nrm, clear=True)
        g.texture_pass(perspective=persp, filter="trilinear", anisotropy=A)
        g.synchronize()
        g.shade_guro(light)
        got = host(f.get_color_tensor())
        assert_bit_equal(got, host(g.get_color_tensor()), f"fused light vs pass + illumination, {persp}")
        want = _want(ref, tri, uv, tex, persp, A, chain=chain, normals=ref.normals_buffer, light_direction=LIGHT)
        assert_bit_equal(got, want, f"fused light vs oracle.guro of the host model, {persp}")
        assert_bit_equal(host(f.get_normals_tensor()), ref.normals_buffer, "normals")
        lit_trilinear = mip_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, persp, chain=chain,
                                             normals=ref.normals_buffer, light_direction=LIGHT)
        assert (want != lit_trilinear).any()
    # the background is shaded too: a colour written there beforehand comes out multiplied
    f.render_arrays(tri, col, nrm, clear=True)
    plane = f.get_color_tensor()
    plane[0, 0, :] = 3.0
    nplane = f.get_normals_tensor()
    nplane[0, 0, 2] = -2.0
    f.texture_pass(filter="trilinear", light_direction=light, anisotropy=A)
    c = ref.color_buffer.copy(); c[0, 0, :] = 3.0
    n = ref.normals_buffer.copy(); n[0, 0, 2] = -2.0
    want = aniso_ref.texture_pass(c, ref.winner, tri, ref.proj_mat, uv, tex, False, A, chain=chain, normals=n,
                                  light_direction=LIGHT)
    assert ref.winner[0, 0] < 0 and want[0, 0, 0] != 0.0 and want[0, 0, 0] != 3.0
    assert_bit_equal(host(f.get_color_tensor()), want, "background under the fused light")


def test_row_strip_leaves_the_other_rows_alone(oracle):
    tri, col, nrm, uv = trex_textured()
    tex = texture(6, 709, 709)
    chain = mip_ref.build_chain(tex)
    H = W = 512
    A = 16
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
        f.texture_pass(filter="trilinear", light_direction=light if with_light else None, anisotropy=A)
        got = host(f.get_color_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        kw = dict(normals=ref.normals_buffer, light_direction=LIGHT) if with_light else {}
        want = _want(ref, tri, uv, tex, False, A, chain=chain, y0=y0, y1=y1, **kw)
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, light={with_light}")
        trilinear = mip_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, chain=chain, y0=y0,
                                         y1=y1, **kw)
        assert (want[y0:y1] != trilinear[y0:y1]).any()


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
    want = _want(ref, tri, uv, tex, True, 8, normals=ref.normals_buffer, light_direction=LIGHT)
    trilinear = mip_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, True,
                                     normals=ref.normals_buffer, light_direction=LIGHT)
    assert (want != trilinear).any()
    f = filler(H, W)
    binds = []
    bind = f.bind_texture
    f.bind_texture = lambda *a, **kw: (binds.append(kw), bind(*a, **kw))[1]
    r = Renderer(f, GuroIllumination(LIGHT), on_device=on_device,
                 texture_pass={"filter": "trilinear", "perspective": True, "anisotropy": 8})
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
    f.render_arrays(tri, col, nrm, clear=True)
    f.texture_pass(filter="trilinear", anisotropy=4)
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match="anisotropy"):
            f.texture_pass(filter="trilinear", anisotropy=bad)
    with pytest.raises(ValueError, match='needs filter="trilinear"'):
        f.texture_pass(filter="bilinear", anisotropy=4)
    # an error of the entry point surfaces with its name: a sample count it refuses, before any launch
    d_uv, _ = f._texture
    rc = f._lib.crender_aniso_shade(f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), len(tri), None, f._P,
                                    d_uv.data_ptr(), f._mip[0].data_ptr(), 8, 8, None, None, f.color_buffer.data_ptr(),
                                    64, 64, 0, 64, 0, 17, f._stream())
    assert rc == _capi.EINVAL
    with pytest.raises(_capi.CrenderError, match="crender_aniso_shade failed.*crender_aniso_shade: bad argument"):
        _capi.check(rc, "crender_aniso_shade")
    # without the chain: the trilinear filter's own message
    f.bind_texture(uv, tex)
    with pytest.raises(ValueError, match="filter 'trilinear' needs a mip chain"):
        f.texture_pass(filter="trilinear", anisotropy=4)
    chain = filler(64, 64, pipeline=True)
    chain.bind_texture(uv, tex, mipmaps=True)
    with pytest.raises(ValueError, match="swap chain"):
        chain.texture_pass(filter="trilinear", anisotropy=4)
