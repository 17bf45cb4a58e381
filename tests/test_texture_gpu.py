"""The deferred texture pass on the GPU (csrc/texture.hip through AdvancedPixelBufferFiller.texture_pass and
Renderer(texture_pass=...)), bit for bit against the host model of tests/tex_ref.py evaluated on the
oracle's frame (itself pinned in tests/test_texture_cpu.py)."""
import os

import numpy as np
import pytest

import tex_ref
from pass_scenes import GOLDEN, filler, host, oracle_frame, planes_only_read, soup_textured, texture, textured_model, trex_textured
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

MODES = [(False, "nearest"), (True, "nearest"), (False, "bilinear"), (True, "bilinear")]
LIGHT = (0.3, -0.2, 1.0)             # what GuroIllumination is constructed with


def _want(ref, tri, uv, tex, persp=False, filt="nearest", **kw):
    return tex_ref.texture_pass(ref.color_buffer, ref.winner, tri, ref.proj_mat, uv, tex, perspective=persp,
                                bilinear_filter=filt == "bilinear", **kw)


def _check_every_mode(oracle, scene, tex, H, W, what, min_covered=1, **filler_kw):
    tri, col, nrm, uv = scene
    ref = oracle_frame(oracle, tri, col, nrm, H, W)
    covered = int((ref.winner >= 0).sum())
    assert covered >= min_covered, (what, covered)
    f = filler(H, W, **filler_kw)
    f.bind_texture(uv, tex)
    for persp, filt in MODES:
        f.render_arrays(tri, col, nrm, clear=True)
        f.texture_pass(perspective=persp, filter=filt)
        want = _want(ref, tri, uv, tex, persp, filt)
        assert not np.isnan(want).any(), (what, persp, filt)
        assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour, perspective={persp}, {filt}")
        if covered:
            assert (want.view(np.uint32) != ref.color_buffer.view(np.uint32)).any(), (what, "the pass changed nothing")
        planes_only_read(f, ref, what)
    return f


@pytest.mark.parametrize("size", [256, 1024, 4096])
def test_trex_every_mode(oracle, size):
    _check_every_mode(oracle, trex_textured(), texture(1, 709, 709), size, size, f"trex{size}", min_covered=15000)


def test_cube_every_mode(oracle):
    from cython3dmodelrenderer_amd import scenes
    tri, col, nrm = scenes.load_fixture("cube_inputs.npz")
    uv = np.random.default_rng(2).uniform(-0.5, 1.5, (len(tri), 3, 2)).astype(np.float32)
    _check_every_mode(oracle, (tri, col, nrm, uv), texture(2, 3, 1000), 256, 256, "cube256", min_covered=1000)


@pytest.mark.parametrize("seed,T,H,W,th,tw", [(31, 4000, 200, 173, 1, 1), (32, 2500, 333, 512, 3, 1000),
                                              (33, 30000, 512, 509, 709, 709), (34, 60, 64, 41, 2, 5)])
def test_random_soups_with_uv_beyond_the_unit_square(oracle, seed, T, H, W, th, tw):
    scene = soup_textured(seed, T, max(H, W), size_px=(1.0, 60.0))
    _check_every_mode(oracle, scene, texture(seed, th, tw), H, W, f"soup{seed}", min_covered=H * W // 20)


def test_presort_gives_the_same_bits(oracle):
    scene = soup_textured(41, 20000, 512, size_px=(2.0, 30.0))
    f = _check_every_mode(oracle, scene, texture(41, 64, 97), 512, 512, "presorted soup", presort=True)
    assert f._order is not None          # the resident inputs are the tile-coherent copy: the pass went through pos_of


def test_fused_light_equals_the_pass_plus_the_illumination(oracle):
    tri, col, nrm, uv = trex_textured()
    tex = texture(5, 709, 709)
    H = W = 1024
    ref = oracle_frame(oracle, tri, col, nrm, H, W)
    light = [float(v) for v in oracle.guro_light(LIGHT)]
    f, g = filler(H, W), filler(H, W)
    f.bind_texture(uv, tex)
    g.bind_texture(uv, tex)
    for persp, filt in MODES:
        f.render_arrays(tri, col, nrm, clear=True)
        f.texture_pass(perspective=persp, filter=filt, light_direction=light)
        g.render_arrays(tri, col, nrm, clear=True)
        g.texture_pass(perspective=persp, filter=filt)
        g.synchronize()
        g.shade_guro(light)
        got = host(f.get_color_tensor())
        assert_bit_equal(got, host(g.get_color_tensor()), f"fused light vs pass + illumination, {persp}, {filt}")
        want = _want(ref, tri, uv, tex, persp, filt, normals=ref.normals_buffer, light_direction=LIGHT)
        assert_bit_equal(got, want, f"fused light vs oracle.guro of the reference, {persp}, {filt}")
        assert_bit_equal(host(f.get_normals_tensor()), ref.normals_buffer, "normals")
    # the background is shaded too: a colour written there beforehand comes out multiplied
    f.render_arrays(tri, col, nrm, clear=True)
    plane = f.get_color_tensor()
    plane[0, 0, :] = 3.0
    nplane = f.get_normals_tensor()
    nplane[0, 0, 2] = -2.0
    f.texture_pass(light_direction=light)
    c = ref.color_buffer.copy(); c[0, 0, :] = 3.0
    n = ref.normals_buffer.copy(); n[0, 0, 2] = -2.0
    want = tex_ref.texture_pass(c, ref.winner, tri, ref.proj_mat, uv, tex, normals=n, light_direction=LIGHT)
    assert want[0, 0, 0] != 0.0 and want[0, 0, 0] != 3.0
    assert_bit_equal(host(f.get_color_tensor()), want, "background under the fused light")


def test_row_strip_leaves_the_other_rows_alone(oracle):
    tri, col, nrm, uv = trex_textured()
    tex = texture(6, 709, 709)
    H = W = 512
    y0, y1 = 135, 301                    # not multiples of the kernel's 8-row blocks
    ref = oracle_frame(oracle, tri, col, nrm, H, W, y0=y0, y1=y1)
    light = [float(v) for v in oracle.guro_light(LIGHT)]
    for with_light in (False, True):
        f = filler(H, W, row_strip=(y0, y1))
        f.bind_texture(uv, tex)
        f.render_arrays(tri, col, nrm, clear=True)
        f.synchronize()
        # rows outside the strip: colours to be kept, and winners that WOULD be textured if the pass looked at them
        f.color_buffer[:y0] = 7.5
        f.color_buffer[y1:] = -2.25
        f.winner_buffer[:y0] = 0
        f.winner_buffer[y1:] = 1
        f.texture_pass(filter="bilinear", light_direction=light if with_light else None)
        got = host(f.get_color_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        kw = dict(normals=ref.normals_buffer, light_direction=LIGHT) if with_light else {}
        want = _want(ref, tri, uv, tex, False, "bilinear", y0=y0, y1=y1, **kw)
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, light={with_light}")


def test_numpy_torch_and_device_model_inputs_agree(oracle):
    import torch
    from cython3dmodelrenderer_amd import scenes
    from cython3dmodelrenderer_amd.data_structures.device_model import DeviceModel
    from cython3dmodelrenderer_amd.data_structures.model import Model
    with np.load(os.path.join(GOLDEN, "trex_mesh.npz")) as z:
        vertices, faces = z["vertices"], z["faces"]
    with np.load(os.path.join(GOLDEN, "trex_uv.npz")) as z:
        uv_pool, faces_uv = z["uv"], z["faces_uv"]
    tex = texture(7, 709, 709)
    m = Model(vertices, faces, uv_pool, faces_uv, tex)
    scenes.fit_model(m)
    H = W = 512
    tri, col, nrm = m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles
    uv = m.get_texture_coords_by_triangles()
    assert uv.shape == (len(tri), 3, 2) and uv.dtype == np.float32 and m.get_texture() is m._texture
    ref = oracle_frame(oracle, tri, col, nrm, H, W)
    assert int((ref.winner >= 0).sum()) > 5000
    want = _want(ref, tri, uv, tex, True, "bilinear")

    a = filler(H, W)                              # numpy
    a.bind_texture(uv, tex)
    a.render_model(m, clear=True)
    a.texture_pass(perspective=True, filter="bilinear")
    assert_bit_equal(host(a.get_color_tensor()), want, "numpy inputs")

    b = filler(H, W)                              # caller's device tensors
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tri, col, nrm)]
    b.bind_texture(torch.from_numpy(uv).cuda(), torch.from_numpy(tex).cuda())
    b.render_arrays(*dev, clear=True)
    b.texture_pass(perspective=True, filter="bilinear")
    assert_bit_equal(host(b.get_color_tensor()), want, "torch inputs")

    dm = DeviceModel(m)                            # the device-resident model's own uv and texture
    duv, dtex = dm.get_texture_coords_by_triangles(), dm.get_texture()
    assert duv.is_cuda and dtex.is_cuda and duv.dtype == torch.float32 and dtex.dtype == torch.uint8
    assert_bit_equal(host(duv), uv, "DeviceModel uv")
    assert np.array_equal(host(dtex), tex)
    c = filler(H, W)
    c.bind_texture(duv, dtex)
    c.render_model(dm, clear=True)
    c.texture_pass(perspective=True, filter="bilinear")
    assert_bit_equal(host(c.get_color_tensor()), want, "DeviceModel inputs")
    # dropping the texture
    c.bind_texture(None, None)
    with pytest.raises(ValueError, match="no texture is bound"):
        c.texture_pass()
    untextured = DeviceModel(Model(vertices[:3], np.arange(3).reshape(1, 3)))
    assert untextured.get_texture_coords_by_triangles() is None and untextured.get_texture() is None


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
    want = _want(ref, tri, uv, tex, True, "bilinear", normals=ref.normals_buffer, light_direction=LIGHT)
    f = filler(H, W)
    binds = []
    bind = f.bind_texture
    f.bind_texture = lambda *a: (binds.append(1), bind(*a))[1]
    r = Renderer(f, GuroIllumination(LIGHT), on_device=on_device, texture_pass={"perspective": True, "filter": "bilinear"})
    for _ in range(2):                             # every frame starts from cleared buffers: the same image twice
        out = r.render(m)
        got = host(out) if on_device in (True, "fused") else np.array(out)
        assert_bit_equal(got, want, f"Renderer(on_device={on_device!r})")
    assert len(binds) == 1                         # the texture went up once per model, not per frame
    assert_bit_equal(host(f.get_normals_tensor()), ref.normals_buffer, "normals")
    # the default stays the reference's image
    plain = Renderer(filler(H, W), GuroIllumination(LIGHT), on_device=on_device)
    out = plain.render(m)
    got = host(out) if on_device in (True, "fused") else np.array(out)
    c = ref.color_buffer.copy()
    oracle.guro(c, ref.normals_buffer, LIGHT)
    assert_bit_equal(got, c, f"Renderer(on_device={on_device!r}) without a texture pass")


def test_host_views_show_the_textured_colours_at_the_next_getter_call(oracle):
    tri, col, nrm, uv = soup_textured(9, 2000, 128, size_px=(3.0, 40.0))
    tex = texture(9, 16, 16)
    ref = oracle_frame(oracle, tri, col, nrm, 128, 128)
    f = filler(128, 128)
    f.bind_texture(uv, tex)
    f.render_arrays(tri, col, nrm, clear=True)
    view = f.get_color_buffer()
    assert_bit_equal(view, ref.color_buffer, "before the pass")
    f.texture_pass()
    again = f.get_color_buffer()
    assert again is view
    assert_bit_equal(view, _want(ref, tri, uv, tex), "after the pass")


def test_a_frame_without_triangles_keeps_its_cleared_colours(oracle):
    e = np.zeros((0, 3, 3), np.float32)
    f = filler(96, 80)
    f.bind_texture(np.zeros((0, 3, 2), np.float32), texture(10, 4, 4))
    light = [float(v) for v in oracle.guro_light(LIGHT)]
    for kw in ({}, {"light_direction": light}, {"perspective": True, "filter": "bilinear"}):
        f.render_arrays(e, e, e, clear=True)
        f.texture_pass(**kw)
        assert (host(f.get_color_tensor()).view(np.uint32) == 0).all(), kw
        assert (host(f.get_winner_tensor()) == -1).all()
    # and a frame whose triangles all miss the view
    tri, col, nrm, uv = soup_textured(10, 50, 96)
    tri[..., 0] += 100.0
    f.bind_texture(uv, texture(10, 4, 4))
    f.render_arrays(tri, col, nrm, clear=True)
    f.texture_pass(filter="bilinear")
    assert (host(f.get_color_tensor()).view(np.uint32) == 0).all()


def test_nan_and_infinite_uv_follow_the_statement(oracle):
    tri, col, nrm, uv = soup_textured(12, 1500, 160, size_px=(4.0, 40.0))
    rng = np.random.default_rng(12)
    odd = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 2147483648.0, -2147483904.0, 1e-42])
    hit = rng.uniform(size=uv.shape) < 0.15
    uv[hit] = rng.choice(odd, int(hit.sum()))
    tex = texture(12, 5, 7)
    ref = oracle_frame(oracle, tri, col, nrm, 160, 160)
    f = filler(160, 160)
    f.bind_texture(uv, tex)
    for persp, filt in MODES:
        f.render_arrays(tri, col, nrm, clear=True)
        f.texture_pass(perspective=persp, filter=filt)
        got = host(f.get_color_tensor())
        want = _want(ref, tri, uv, tex, persp, filt)
        # (IEEE 754 leaves the sign and payload of a generated NaN open: x86 and gfx950 differ there)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (persp, filt)
        assert_bit_equal(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), f"odd uv, {persp}, {filt}")
        if filt == "nearest":
            assert not nan.any()         # the cast sends every odd coordinate to texel 0 or the far edge
        else:
            assert nan.any()


def test_errors_name_their_cause(oracle):
    from cython3dmodelrenderer_amd.data_structures.model import Model
    from cython3dmodelrenderer_amd.illumination.guro_illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    tri, col, nrm, uv = soup_textured(13, 300, 64)
    tex = texture(13, 8, 8)
    f = filler(64, 64, track_winner=False)
    f.bind_texture(uv, tex)
    f.render_arrays(tri, col, nrm, clear=True)
    with pytest.raises(ValueError, match="winner plane"):
        f.texture_pass()
    f = filler(64, 64)
    with pytest.raises(ValueError, match="no frame has been rendered|no texture is bound"):
        f.texture_pass()
    f.render_arrays(tri, col, nrm, clear=True)
    with pytest.raises(ValueError, match="no texture is bound"):
        f.texture_pass()
    f.bind_texture(uv[:-1], tex)
    with pytest.raises(ValueError, match="299 triangles of texture coordinates are bound, the last frame drew 300"):
        f.texture_pass()
    f.bind_texture(uv, tex)
    with pytest.raises(ValueError, match="filter"):
        f.texture_pass(filter="trilinear")
    f.render_arrays(tri, col, nrm)                 # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.texture_pass()
    f.render_arrays(tri, col, nrm, clear=True)
    f.texture_pass()                               # and works again
    for bad in ((None, tex), (uv, None), (uv.astype(np.float64), tex), (uv[:, :, :1], tex), (uv, tex.astype(np.float32)),
                (uv, tex[:, :, :2])):
        with pytest.raises(ValueError):
            f.bind_texture(*bad)
    chain = filler(64, 64, pipeline=True)
    chain.bind_texture(uv, tex)
    with pytest.raises(ValueError, match="swap chain"):
        chain.texture_pass()
    T = len(tri)
    idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    plain = Model(tri.reshape(-1, 3), idx, normals=nrm.reshape(-1, 3), triangles_normals=idx, recalculate_normals=False)
    plain.set_uniform_color()
    with pytest.raises(ValueError, match="textured model"):
        Renderer(filler(64, 64), GuroIllumination(LIGHT), texture_pass={}).render(plain)


def test_a_frame_redrawn_after_a_bin_overflow_ends_textured(oracle):
    """The scene of test_filler_recovers_from_bin_overflow: the bin lists are far too small, the frame drops
    fragments and is rendered again when it is settled — which the pass does before it launches."""
    rng = np.random.default_rng(21)
    tri, col, nrm = random_soup(rng, 400, 512, size_px=(150, 400), frac_backface=0.0)
    uv = rng.uniform(-0.5, 1.5, (400, 3, 2)).astype(np.float32)
    tex = texture(21, 31, 17)
    ref = oracle_frame(oracle, tri, col, nrm, 512, 512)
    for presort in (False, True):
        f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False, presort=presort)
        f.bind_texture(uv, tex)
        f.render_arrays(tri, col, nrm, clear=True)
        need, cap = f.bin_usage()
        assert cap == 500 and need > cap and len(f._pending) == 1      # this frame dropped fragments, nobody has looked yet
        f.texture_pass(perspective=True)
        assert not f._pending and f.bin_usage()[1] >= need             # grown and redone before the pass
        assert_bit_equal(host(f.get_color_tensor()), _want(ref, tri, uv, tex, True), f"redone frame, presort={presort}")
        assert_bit_equal(host(f.get_winner_tensor()), ref.winner, "winner")
        assert_bit_equal(host(f.get_z_tensor()), ref.z_buffer, "z")
