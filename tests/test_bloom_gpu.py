"""Bloom and tone mapping on the GPU (csrc/bloom.hip's k_bloom_rows and k_bloom_finish through the fillers' ``bloom``,
the C entry, ``bloom.bloom`` and Renderer(bloom=...)), bit for bit against the host model of tests/bloom_ref.py, the
scratch plane included, on the oracle's frames and on hand-built images (the model is pinned in tests/test_bloom_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import bloom_ref
import phong_ref
from pass_scenes import Scene, TriangleModel, filler, host, lib, soup_fixture, trex_arrays, trex_fixture  # noqa: F401
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)
INF = float("inf")


class _Scene(Scene):
    def check(self, f, what, counts=None, **kw):
        """Draw, bloom through the filler, compare the image and the scratch plane with the model."""
        self.draw(f)
        out = f.bloom(**kw)
        hb = np.zeros_like(self.cam.color_buffer)
        want = bloom_ref.bloom(self.cam.color_buffer, counts=counts, scratch=hb, **kw)
        assert tuple(out.shape) == (self.H, self.W, 3) and out.data_ptr() != f.color_buffer.data_ptr()
        assert str(out.dtype) == "torch." + kw.get("dtype", "float32")
        assert_bit_equal(host(out), want, f"{what}: the image")
        assert_bit_equal(host(f._bloom_scratch[(self.H, self.W)]), hb, f"{what}: the scratch plane")
        assert_bit_equal(host(f.get_color_tensor()), self.cam.color_buffer, f"{what}: the colour plane is only read")
        self.check_planes(f, what)
        return want


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


@pytest.fixture(scope="module")
def filler256():
    return filler(256, 256)


# ---- 1. T-Rex and the soup at 256 x 256 ------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 8, 32])
@pytest.mark.parametrize("scene", ["trex", "soup"])
def test_scenes_at_every_radius(trex256, soup256, filler256, scene, R):
    s = trex256 if scene == "trex" else soup256
    counts = {}
    want = s.check(filler256, f"{scene}, radius {R}", counts=counts, threshold=bloom_ref.PINNED_THRESHOLD[scene], radius=R)
    print(f"{scene}, radius {R}: {counts}")
    assert (counts["bright"], counts["copied"], counts["glow"]) == bloom_ref.PINNED_COUNTS[scene, R]
    # (a glow below half an ulp of its pixel leaves the bits: a few pixels at the rim)
    assert 0.99 * counts["glow"] <= s.assert_changed(want, scene).sum() <= counts["glow"]


@pytest.mark.parametrize("scene", ["trex", "soup"])
def test_scenes_tone_mapped(trex256, soup256, filler256, scene):
    s = trex256 if scene == "trex" else soup256
    thr = bloom_ref.PINNED_THRESHOLD[scene]
    for kw in (dict(tonemap="reinhard"), dict(gamma=2), dict(dtype="uint8"), dict(flip_rows=True), dict(exposure=1.75),
               dict(tonemap="reinhard", white=1.5, gamma=2, dtype="uint8", flip_rows=True, exposure=1.25, intensity=2.5),
               dict(tonemap="reinhard", white=0.75, clamp=200.0), dict(dtype="uint8", clamp=300.0, intensity=3.0)):
        want = s.check(filler256, f"{scene}, {kw}", threshold=thr, radius=8, **kw)
        assert len(np.unique(want)) > 50
    plain = bloom_ref.bloom(s.cam.color_buffer, threshold=thr, radius=8)
    assert_bit_equal(bloom_ref.bloom(s.cam.color_buffer, threshold=thr, radius=8, flip_rows=True), plain[::-1], "flipped")


# ---- 2. hand-built images through the C entry ------------------------------------------------------------------

def device_bloom(src, y0=0, y1=None, out=None, scratch=None, **kw):
    """(the result plane, the scratch plane) of crender_bloom over rows y0 .. y1 of `src`; rows outside are `out`'s and
    `scratch`'s, NaN (or 0xAB bytes) without them.  The source is checked to be only read."""
    import torch
    from cython3dmodelrenderer_amd import _capi, bloom
    call = bloom.arguments(**kw)
    H, W = src.shape[:2]
    src = np.ascontiguousarray(src, np.float32)
    d_src = torch.from_numpy(src).cuda()
    if out is None:
        out = np.full((H, W, 3), 0xAB, np.uint8) if call.dtype == "uint8" else np.full((H, W, 3), np.nan, np.float32)
    d_out = torch.from_numpy(np.ascontiguousarray(out)).cuda()
    d_scratch = torch.from_numpy(np.full((H, W, 3), np.nan, np.float32) if scratch is None else np.ascontiguousarray(scratch)).cuda()
    bloom.launch(_capi.load(), d_src, d_scratch, d_out, call, y0, H if y1 is None else y1,
                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    got = host(d_out), host(d_scratch)
    assert_bit_equal(host(d_src), src, "the source is only read")
    return got


def check_image(src, what, min_glow=1, min_copied=0, **kw):
    """The C entry against the model, image and scratch plane, rows outside the strip untouched; -> the model's counts."""
    H, W = src.shape[:2]
    u8 = kw.get("dtype") == "uint8"
    start = np.full((H, W, 3), 0xAB, np.uint8) if u8 else np.full((H, W, 3), np.nan, np.float32)
    counts, hb = {}, np.full((H, W, 3), np.nan, np.float32)
    want = bloom_ref.bloom(src, counts=counts, scratch=hb, out=start.copy(), **kw)
    assert counts["glow"] >= min_glow and counts["copied"] >= min_copied, (what, counts)
    got, got_hb = device_bloom(src, **kw)
    assert_bit_equal(got, want, f"{what}: the image")
    assert_bit_equal(got_hb, hb, f"{what}: the scratch plane")
    return counts


def sparse_image(seed, H, W, share=0.05, top=600.0, dark=250.0):
    """Mostly below 255, a share of the pixels up to `top`."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, dark, (H, W, 3)).astype(np.float32)
    hot = rng.uniform(size=(H, W)) < share
    img[hot] = rng.uniform(200.0, top, (int(hot.sum()), 3)).astype(np.float32)
    return img


# 5 x 7, 1 x 40 and 40 x 1: frames smaller than the halo.  33 x 65: one pixel taller and one pixel wider than whole tiles
# of 32.  63 x 31: a partial tile in both directions.
@pytest.mark.parametrize("H,W", [(5, 7), (1, 40), (40, 1), (33, 65), (63, 31)])
def test_frames_that_do_not_fit_the_tiles(H, W):
    for R in (1, 32):
        for share in (0.5, 0.06):
            img = sparse_image(80 + H + R, H, W, share=share)
            img[H // 2, W // 2] = np.float32([500.0, 20.0, 300.0])
            check_image(img, f"{H} x {W}, radius {R}, share {share}", threshold=255.0, radius=R)
            check_image(img, f"{H} x {W}, radius {R}, share {share}, uint8 flipped", threshold=255.0, radius=R, dtype="uint8",
                        flip_rows=True, tonemap="reinhard")
            if H > 8:
                check_image(img, f"{H} x {W}, radius {R}, rows 3 .. {H - 2}", threshold=255.0, radius=R, y0=3, y1=H - 2)
                check_image(img, f"{H} x {W}, radius {R}, rows 3 .. {H - 2}, flipped", threshold=255.0, radius=R, y0=3, y1=H - 2,
                            flip_rows=True, gamma=2)


def test_a_frame_of_more_tiles_than_the_grid_holds():
    """A launch is at most 2048 workgroups, each looping over tiles of 32 x 32: a frame 3 pixels wide and 65 600 tall is
    2050 tiles, so two workgroups make a second trip."""
    img = sparse_image(91, 65600, 3, share=0.02)
    img[65590, 1] = np.float32([900.0, 800.0, 100.0])
    counts = check_image(img, "65600 x 3", threshold=255.0, radius=2, min_glow=1000, min_copied=1000)
    assert counts["bright"] > 500
    want = bloom_ref.bloom(img, threshold=255.0, radius=2)
    assert (want[65536:].view(np.uint32) != img[65536:].view(np.uint32)).any()          # the second trip's rows


def test_dark_tiles_beside_bright_tiles():
    """96 x 96: the left two columns of tiles dark (odd values included), the right one bright.  The dark pixels within
    `radius` columns of the bright ones glow, the rest are copied bit for bit; at radius 32 the leftmost tiles stage
    nothing bright in either kernel and skip their walks, at 1 and 8 the middle ones take their halo from the bright tile."""
    rng = np.random.default_rng(5)
    img = rng.uniform(-50.0, 250.0, (96, 96, 3)).astype(np.float32)
    img[:, 64:] = rng.uniform(256.0, 700.0, (96, 32, 3)).astype(np.float32)
    img[10, 3] = np.float32([-0.0, np.nan, -np.inf])
    img[40, 50].view(np.uint32)[:] = [0x7FC00123, 0xFFC00001, 0x80000000]
    for R in (1, 8, 32):
        mask = np.zeros((96, 96), bool)
        want = bloom_ref.bloom(img, threshold=255.0, radius=R, mask=mask)
        changed = (want.view(np.uint32) != img.view(np.uint32)).any(2)
        # the model says so: the glow reaches R columns into the dark side and no further
        assert mask[:, 64 - R:].all() and not mask[:, :64 - R].any() and not changed[:, :64 - R].any()
        assert changed[:, 64 - R:64].mean() > 0.95
        assert_bit_equal(want[:, :64 - R], img[:, :64 - R], f"radius {R}: the model copies what no glow reaches")
        check_image(img, f"dark beside bright, radius {R}", threshold=255.0, radius=R, min_glow=96 * (32 + R), min_copied=96 * (64 - R))
    # and the other way round in y: bright rows above dark rows, through the column pass alone
    check_image(np.ascontiguousarray(img.transpose(1, 0, 2)), "dark below bright, radius 32", threshold=255.0, radius=32,
                min_copied=96 * 32)


# ---- 3. special values -----------------------------------------------------------------------------------------

def _assert_equal_up_to_computed_nans(got, want, computed_at, what):
    """Bit for bit, but where the model COMPUTED a NaN: there the kernel has a NaN as well, whose sign and payload the
    contract leaves open (the host's and the device's differ).  A copied pixel keeps every bit of its NaNs."""
    computed = np.isnan(want) & computed_at
    assert np.isnan(got[computed]).all(), what
    assert_bit_equal(np.where(computed, np.float32(0), got), np.where(computed, np.float32(0), want), what)


def _odd_image(seed, H, W, plus_inf=True):
    rng = np.random.default_rng(seed)
    img = sparse_image(seed, H, W, share=0.04)
    hit = rng.uniform(size=(H, W)) < 0.06
    values = [np.nan, -np.inf, -0.0, -17.5, 1e-42] + ([np.inf] if plus_inf else [])
    img[hit] = rng.choice(np.float32(values), (int(hit.sum()), 3))
    img[1, 1].view(np.uint32)[:] = [0x7FC00123, 0xFFC00001, 0x80000000]             # NaN payloads and a -0
    return img


def test_special_values_through_the_c_entry():
    H, W = 70, 45
    img = _odd_image(61, H, W)
    assert np.isinf(img).any() and np.isnan(img).any()
    seen = dict(computed=False, copied=False)
    zero_tail = np.float32([0.5, 0.25, 0.0, 0.0, 0.0])                    # zero weights: 0 * inf is a NaN
    for kw in (dict(radius=1), dict(radius=8), dict(weights=zero_tail), dict(weights=zero_tail, tonemap="reinhard", gamma=2),
               dict(radius=3, exposure=0.0), dict(radius=3, clamp=-INF), dict(radius=2, intensity=1e30),
               dict(radius=2, intensity=1e-44), dict(radius=4, white=1e-30, tonemap="reinhard")):
        mask, hb = np.zeros((H, W), bool), np.zeros_like(img)
        want = bloom_ref.bloom(img, threshold=255.0, mask=mask, scratch=hb, **kw)
        seen["computed"] |= bool(np.isnan(want[mask]).any())
        seen["copied"] |= bool(np.isnan(want[~mask]).any())
        assert mask.sum() > 50
        got, got_hb = device_bloom(img, threshold=255.0, **kw)
        everywhere = np.ones((H, W, 3), bool)
        _assert_equal_up_to_computed_nans(got_hb, hb, everywhere, f"odd values, {kw}: the scratch plane")
        # what the tone stage computes from a copied NaN is computed too; without the stage a copied NaN keeps its bits
        toned = any(k in kw for k in ("tonemap", "gamma", "exposure"))
        _assert_equal_up_to_computed_nans(got, want, everywhere if toned else np.broadcast_to(mask[..., None], got.shape),
                                          f"odd values, {kw}")
    assert seen == dict(computed=True, copied=True)                  # NaNs that were computed, and NaNs that were copied
    # uint8 of the odd values: a NaN and what is out of range give INT_MIN's low byte, 0
    mask = np.zeros((H, W), bool)
    want = bloom_ref.bloom(img, threshold=255.0, radius=2, dtype="uint8", clamp=INF, mask=mask)
    assert np.array_equal(device_bloom(img, threshold=255.0, radius=2, dtype="uint8", clamp=INF)[0], want)
    # intensity 0 keeps every bit, a -0 within a glow's reach too.  (Without +inf: a bright pixel with an infinite channel
    # has q = inf / inf, its glow is a NaN, and 0 times a NaN is not 0.)
    odd = _odd_image(62, H, W, plus_inf=False)
    for R in (1, 8, 32):
        c = {}
        bloom_ref.bloom(odd, threshold=255.0, radius=R, counts=c)
        assert c["bright"] > 50 and c["glow"] > 500
        assert_bit_equal(device_bloom(odd, threshold=255.0, radius=R, intensity=0.0)[0], odd, f"intensity 0, radius {R}")
        assert_bit_equal(bloom_ref.bloom(odd, threshold=255.0, radius=R, intensity=0.0), odd, f"the model, intensity 0, radius {R}")
    # a threshold above every finite pixel, and +inf: copies
    assert_bit_equal(device_bloom(odd, threshold=1e30, radius=8)[0], odd, "a threshold above every pixel")
    assert_bit_equal(device_bloom(img, threshold=INF, radius=8)[0], img, "a threshold of +inf")
    # a threshold of 0: every pixel with a positive channel is bright by all of its colour (q = 1)
    c = check_image(odd, "threshold 0", threshold=0.0, radius=3, min_glow=H * W // 2)
    assert c["bright"] > 0.9 * H * W
    black = np.zeros((40, 40, 3), np.float32)
    black[5, 5, 1] = -0.0
    assert_bit_equal(device_bloom(black, threshold=0.0, radius=8)[0], black, "threshold 0 over black: nothing is bright")


# ---- 4. a row strip --------------------------------------------------------------------------------------------

def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_zero(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    s.draw(f)
    f.synchronize()
    # rows outside the strip: colours that WOULD glow if the pass read them
    f.color_buffer[:y0] = 7.5e3
    f.color_buffer[y1:] = float("nan")
    kw = dict(threshold=100.0, radius=8)
    counts = {}
    want = bloom_ref.bloom(s.cam.color_buffer, y0=y0, y1=y1, counts=counts, **kw)
    assert counts["glow"] > 1000 and counts["copied"] > 1000
    got = host(f.bloom(**kw))
    assert not got[:y0].any() and not got[y1:].any()
    assert_bit_equal(got, want, "the strip's rows")
    # flipped and as bytes: the strip lands in rows H - y1 .. H - y0, the others stay zero
    flipped = host(f.bloom(flip_rows=True, dtype="uint8", **kw))
    assert not flipped[:200 - y1].any() and not flipped[200 - y0:].any() and flipped[200 - y1:200 - y0].any()
    assert np.array_equal(flipped, bloom_ref.bloom(s.cam.color_buffer, y0=y0, y1=y1, flip_rows=True, dtype="uint8", **kw))
    # the poison works: a pass that looked across the strip's edge would give other colours
    seen = bloom_ref.bloom(host(f.get_color_tensor()), **kw)
    assert (seen[y0:y1].view(np.uint32) != want[y0:y1].view(np.uint32)).any()
    assert_bit_equal(host(f.get_color_tensor())[y0:y1], s.cam.color_buffer[y0:y1], "the colour plane is only read")


# ---- 5. host edits and fillers ---------------------------------------------------------------------------------

KW = dict(threshold=200.0, radius=6, intensity=1.5)


def test_host_view_edits_reach_the_pass(soup256, filler256):
    s, f = soup256, filler256
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    want = bloom_ref.bloom(s.cam.color_buffer, **KW)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(f.bloom(**KW)), want, "the plain pass")
    assert f.get_color_buffer() is view
    assert_bit_equal(view, s.cam.color_buffer, "the view still shows the frame")
    view[100:104, 100:140] = np.float32([1000.0, 100.0, 2000.0])
    edited = s.cam.color_buffer.copy()
    edited[100:104, 100:140] = np.float32([1000.0, 100.0, 2000.0])
    want_c = bloom_ref.bloom(edited, **KW)
    assert (want_c != want).any()
    assert_bit_equal(host(f.bloom(**KW)), want_c, "over edited colours")
    assert_bit_equal(host(f.get_color_tensor()), edited, "the colour plane holds the edit and is only read")


def test_a_frame_redrawn_after_a_bin_overflow_ends_bloomed(oracle):
    """The scene of test_a_frame_redrawn_after_a_bin_overflow_ends_lit: the bin lists are far too small, the frame drops
    fragments and is rendered again when it is settled — which the pass does before it hands the plane to the kernel."""
    s = _Scene(oracle, random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0), 512, 512)
    want = bloom_ref.bloom(s.cam.color_buffer, **KW)
    assert (want != s.cam.color_buffer).any()
    f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False)
    s.draw(f)
    need, cap = f.bin_usage()
    assert cap == 500 and need > cap and len(f._pending) == 1     # dropped fragments, nobody has looked yet
    out = f.bloom(**KW)
    assert not f._pending                                          # grown and redone
    assert_bit_equal(host(out), want, "a redone frame")
    s.check_planes(f, "a redone frame")


def test_the_wireframe_filler_glows():
    from cython3dmodelrenderer_amd import scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import EdgeOnlyPixelBufferFiller, LineBresenham
    size = 256
    tri, col, nrm = trex_arrays()
    model = TriangleModel(scenes.fit_soup_to_frame(tri, size, size), col, nrm)
    f = EdgeOnlyPixelBufferFiller(LineBresenham(), (600.0, 128.0, 300.0), h=size, w=size, device="cuda:0")
    f.render_model(model)
    lines = host(f.get_color_tensor())
    drawn = (lines != 0).any(axis=2)
    assert 0.01 < drawn.mean() < 0.5
    counts = {}
    want = bloom_ref.bloom(lines, radius=4, counts=counts)
    assert counts["bright"] == drawn.sum() and counts["glow"] > 1.5 * counts["bright"] and counts["copied"] > 1000
    assert_bit_equal(host(f.bloom(radius=4)), want, "bright lines on black")
    png = f.bloom(radius=4, tonemap="reinhard", dtype="uint8", flip_rows=True)
    assert np.array_equal(host(png), bloom_ref.bloom(lines, radius=4, tonemap="reinhard", dtype="uint8", flip_rows=True))
    assert_bit_equal(host(f.get_color_tensor()), lines, "the colour plane is only read")


def test_bloom_after_pipelined_frames():
    tri, col, nrm = trex_arrays()
    f = filler(256, 256, pipeline=True)
    f.render_arrays(tri, col, nrm, clear=True)
    for _ in range(3):
        f.render_frame()
    got = host(f.bloom(threshold=100.0, radius=5))
    color = host(f.get_color_tensor())
    want = bloom_ref.bloom(color, threshold=100.0, radius=5)
    assert (color != 0).any() and (want != color).any()
    assert_bit_equal(got, want, "the most recently submitted frame, bloomed")


def test_the_free_function(soup256):
    import torch
    from cython3dmodelrenderer_amd import bloom
    src = np.ascontiguousarray(soup256.cam.color_buffer[:100, :77])
    t = torch.from_numpy(src).cuda()
    with torch.cuda.stream(torch.cuda.Stream()):
        out = bloom.bloom(t, threshold=180.0, radius=12, gamma=2)
        torch.cuda.current_stream().synchronize()
    assert out.data_ptr() != t.data_ptr() and tuple(out.shape) == (100, 77, 3)
    assert_bit_equal(host(out), bloom_ref.bloom(src, threshold=180.0, radius=12, gamma=2), "bloom.bloom on a stream of its own")
    assert_bit_equal(host(t), src, "the image is only read")


# ---- 6. source= and the Renderer -------------------------------------------------------------------------------

DOF = dict(focus=0.8473, aperture=20.0, band=0.1, max_radius=6)
B = dict(threshold=150.0, radius=6, intensity=1.25, tonemap="reinhard", white=1.2)


def test_bloom_follows_each_of_the_four_last_passes(soup256):
    s = soup256
    f = filler(256, 256)
    s.draw(f)
    results = {"depth_of_field": f.depth_of_field(**DOF), "edge_aa": f.edge_aa(),
               "transparency_pass": f.transparency_pass(0.5, layers=3), "resolve": f.resolve(2)}
    for name, t in results.items():
        src = host(t)
        want = bloom_ref.bloom(src, **B)
        assert (want != src).any(), name
        out = f.bloom(source=t, **B)
        assert out.data_ptr() != t.data_ptr() and tuple(out.shape) == tuple(t.shape)
        assert_bit_equal(host(out), want, f"bloom(source={name}'s tensor)")
        assert_bit_equal(host(t), src, f"{name}'s tensor is only read")
    assert sorted(f._bloom_scratch) == [(128, 128), (256, 256)]
    s.check_planes(f, "after the passes")
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "the colour plane is only read")


@pytest.mark.parametrize("keyword,value", [("depth_of_field", DOF), ("antialias", {}), ("transparency", dict(alpha=0.5, layers=3)),
                                           ("supersample", 2)])
def test_renderer_combines_bloom_with_each_of_the_four(soup256, keyword, value):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    for on_device in (True, None, "fused"):
        a = filler(256, 256)
        by_hand = Renderer(a, GuroIllumination(GURO), None, 256, 256, on_device=True if on_device is None else on_device,
                           **{keyword: value}).render(s.model)
        src = host(by_hand)
        want = bloom_ref.bloom(src, **B)
        assert (want != src).any()
        assert_bit_equal(host(a.bloom(source=by_hand, **B)), want, f"{keyword}, then bloom by hand")
        f = filler(256, 256)
        r = Renderer(f, GuroIllumination(GURO), None, 256, 256, on_device=on_device, bloom=B, **{keyword: value})
        for _ in range(2):
            out = r.render(s.model)
            assert isinstance(out, np.ndarray) == (on_device is None)
            assert_bit_equal(out if on_device is None else host(out), want, f"Renderer({keyword}=..., bloom=...), on_device={on_device!r}")


PHONG_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.9), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.5)]
PHONG_KW = dict(ambient=0.15, shininess=8)


def test_renderer_blooms_the_highlights_of_a_phong_light(soup256):
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    lit = phong_ref.phong_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.cam.normals_buffer, PHONG_LIGHTS,
                               clamp=INF, **PHONG_KW)
    hot = (lit.max(2) > 255).sum()
    assert hot > 500 and lit.max() > 300                            # highlights above white, which the default clamp would cut
    opts = dict(radius=8, tonemap="reinhard", white=2.0, dtype="uint8", flip_rows=True)
    counts = {}
    want = bloom_ref.bloom(lit, counts=counts, **opts)
    assert counts["bright"] == hot and counts["glow"] > hot and want.dtype == np.uint8
    for on_device in (True, None):
        f = filler(256, 256)
        got = Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, clamp=INF, **PHONG_KW), on_device=on_device, bloom=opts).render(s.model)
        assert np.array_equal(got if on_device is None else host(got), want), on_device
        assert_bit_equal(host(f.get_color_tensor()), lit, "the Phong pass's colours, only read")
    plain = bloom_ref.bloom(lit, radius=8)
    f = filler(256, 256)
    assert_bit_equal(host(Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, clamp=INF, **PHONG_KW), on_device=True,
                                   bloom=dict(radius=8)).render(s.model)), plain, "float32, no tone stage")
    assert (plain.max(2) > 255).sum() > hot                        # the glow adds to what was above white already


def test_renderer_blooms_the_host_forms_edits(soup256, oracle):
    """on_device=False: the illumination runs in numpy on the host views; bloom carries those edits up first."""
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    lit = oracle.guro(s.cam.color_buffer.copy(), s.cam.normals_buffer, GURO)
    want = bloom_ref.bloom(lit, **B)
    f = filler(256, 256)
    got = Renderer(f, GuroIllumination(GURO), on_device=False, bloom=B).render(s.model)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want, equal_nan=True) and (want != lit).any()


# ---- 7. errors -------------------------------------------------------------------------------------------------

def test_errors_name_their_cause_and_leave_the_planes_untouched(soup256, lib):
    import torch
    from cython3dmodelrenderer_amd import _capi
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    f = filler(256, 256)
    s.draw(f)
    for kw, message in ((dict(threshold=-1.0), "threshold must be a number, 0 or above"), (dict(radius=33), "radius must be an int from 1 to 32"),
                        (dict(weights=[1.0, float("nan")]), "weights must be a table of 2 to 33 finite numbers"),
                        (dict(intensity=INF), "intensity must be a finite number"), (dict(exposure=-1.0), "exposure must be a finite number"),
                        (dict(tonemap="aces"), "tonemap must be None, 'none' or 'reinhard'"), (dict(white=0.0), "white must be a number above 0"),
                        (dict(gamma=2.2), "gamma must be 1 or 2"), (dict(clamp=float("nan")), "clamp must be None or a number"),
                        (dict(dtype="float16"), "dtype must be 'float32' or 'uint8'"),
                        (dict(source=torch.zeros((8, 8, 3))), "source must be on the filler's device cuda:0, got cpu"),
                        (dict(source=torch.zeros((8, 8, 3), device="cuda:0", dtype=torch.float64)), "source must be a contiguous float32"),
                        (dict(source=f.color_buffer[:, ::2]), "source must be a contiguous float32")):
        with pytest.raises(ValueError, match=message):
            f.bloom(**kw)
    assert f._bloom_scratch is None                                # nothing was allocated or launched
    with pytest.raises(ValueError, match=r"\['knee'\] unknown"):
        Renderer(f, GuroIllumination(GURO), bloom=dict(knee=0.5))
    with pytest.raises(ValueError, match="object has no bloom"):
        Renderer(object(), GuroIllumination(GURO), bloom={})
    # an error of the entry point surfaces with its text, before any launch: the result may not be the source
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = (C.c_float * 2)(0.5, 0.25)
    scratch = torch.empty_like(f.color_buffer)
    rc = lib.crender_bloom(f.color_buffer.data_ptr(), 255.0, w, 1, 1.0, 1.0, 0.0, INF, scratch.data_ptr(), f.color_buffer.data_ptr(),
                           256, 256, 0, 256, 0, st)
    assert rc == _capi.EINVAL
    with pytest.raises(_capi.CrenderError, match="crender_bloom failed.*are not three planes"):
        _capi.check(rc, "crender_bloom")
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "nothing was written")
    out = f.bloom(**KW)                            # and works again
    want = bloom_ref.bloom(s.cam.color_buffer, **KW)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(out), want, "after the errors")
    s.check_planes(f, "after the errors")
