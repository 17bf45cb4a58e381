"""Transparency on the GPU (csrc/peel.hip's k_peel_seed, k_peel_cover, k_peel_resolve and k_peel_blend through
AdvancedPixelBufferFiller.peel_layers and transparency_pass, the two C entries and Renderer(transparency=...)), bit for bit
against the host model of tests/peel_ref.py (itself pinned in tests/test_peel_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import peel_ref
from pass_scenes import LIGHT, Scene, Soup, filler, host, lib, planes_only_read, soup_fixture, trex_arrays, trex_fixture  # noqa: F401
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GROUND = (10.0, 20.0, 30.0)


class _Scene(Scene):
    """A scene, the oracle's frame of it and, computed once, the model's fragments."""
    _frags = None

    @property
    def frags(self):
        if self._frags is None:
            self._frags = peel_ref.fragments(self.tri, self.nrm, self.cam.proj_mat, self.H, self.W)
        return self._frags

    def want(self, alpha, n, light=None, front=None, background=GROUND, **kw):
        return peel_ref.transparency(self.frags, self.tri, self.col, self.nrm, self.cam.proj_mat, alpha, n, light=light,
                                     background=background, front=front, **kw)


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


@pytest.fixture(scope="module")
def filler256():
    return filler(256, 256)


def _check_layers(f, s, n, what, frags=None, y0=0, y1=None):
    w, z = f.peel_layers(n)
    assert tuple(w.shape) == tuple(z.shape) == (n, s.H, s.W)
    want_w, want_z = peel_ref.layers(s.frags if frags is None else frags, n)
    y1 = s.H if y1 is None else y1
    gw, gz = host(w), host(z)
    assert_bit_equal(gw[:, y0:y1], want_w[:, y0:y1], f"{what}: winners")
    assert_bit_equal(gz[:, y0:y1], want_z[:, y0:y1], f"{what}: z")
    assert_bit_equal(gw[0, y0:y1], host(f.get_winner_tensor())[y0:y1], f"{what}: layer 0 is the frame's winner plane")
    assert_bit_equal(gz[0, y0:y1], host(f.get_z_tensor())[y0:y1], f"{what}: layer 0 is the frame's z plane")
    return gw, gz


# ---- 1. the layers of the two scenes -----------------------------------------------------------------------------

@pytest.mark.parametrize("scene,n", [("trex", 6), ("soup", 8)])
def test_layers_of_the_scenes(trex256, soup256, filler256, scene, n):
    s = trex256 if scene == "trex" else soup256
    s.draw(filler256)
    gw, _ = _check_layers(filler256, s, n, scene)
    per_layer = [int((gw[k] >= 0).sum()) for k in range(n)]
    print(f"{scene}: pixels per layer {per_layer}")
    if scene == "trex":
        assert per_layer == [15801, 3197, 683, 110, 17, 0]
    else:
        assert per_layer == [65439, 64668, 61786, 55946, 46989, 36264, 26171, 17676]
    s.check_planes(filler256, scene)
    assert_bit_equal(host(filler256.get_color_tensor()), s.cam.color_buffer, f"{scene}: the colour plane is only read")


# ---- 2. edge scenes ----------------------------------------------------------------------------------------------

def test_coplanar_duplicates_peel_one_by_one(oracle):
    """One triangle five times: every covered pixel holds five fragments of one z, which differ in the key's low word
    alone.  The frame shows the highest index; the layers behind it count down."""
    H = W = 64
    tri = np.repeat(np.float32([[[-0.3, -0.25, 1.0], [0.32, -0.1, 1.3], [-0.05, 0.33, 0.9]]]), 5, 0)
    nrm = np.repeat(np.float32([[[0.1, 0.2, -1.0], [0.0, -0.3, -0.9], [0.2, 0.0, -0.8]]]), 5, 0)
    col = np.random.default_rng(4).uniform(0, 255, tri.shape).astype(np.float32)
    s = _Scene(oracle, (tri, col, nrm), H, W)
    assert s.covered > 200
    f = filler(H, W)
    s.draw(f)
    gw, gz = _check_layers(f, s, 6, "five copies")
    covered = s.cam.winner >= 0
    for k in range(5):
        assert (gw[k][covered] == 4 - k).all() and (gw[k][~covered] == -1).all(), k
        assert_bit_equal(gz[k], s.cam.z_buffer, f"layer {k}: the same z")
    assert (gw[5] == -1).all() and (gz[5] == np.float32(1e6)).all()
    alpha = np.float32([0.5, 0.25, 1.0, 0.125, 0.75])
    assert_bit_equal(host(f.transparency_pass(alpha, layers=6, background=GROUND, front="model")), s.want(alpha, 6), "blended")


def test_a_triangle_larger_than_the_frame_in_front_of_a_soup(oracle):
    """The box clipped on all four sides and 1024 trips of the 8 x 8 walk for one wavefront."""
    H = W = 256
    tri, col, nrm = random_soup(np.random.default_rng(17), 800, 256, size_px=(3.0, 50.0))
    big = np.float32([[[-9.0, -7.0, 0.3], [9.5, -6.0, 0.3], [0.5, 11.0, 0.3]]])
    tri = np.concatenate([tri[:400], big, tri[400:]])
    col = np.concatenate([col[:400], np.float32([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]]), col[400:]])
    nrm = np.concatenate([nrm[:400], np.float32([[[0, 0, -1]] * 3]), nrm[400:]])
    s = _Scene(oracle, (tri, col, nrm), H, W)
    assert (s.cam.winner == 400).all()                  # the big triangle hides everything
    f = filler(H, W)
    s.draw(f)
    gw, _ = _check_layers(f, s, 4, "the big triangle")
    assert (gw[1] >= 0).sum() > 20000 and not (gw[1:] == 400).any()
    alpha = np.random.default_rng(18).uniform(0, 1, len(tri)).astype(np.float32)
    alpha[400] = 0.25
    assert_bit_equal(host(f.transparency_pass(alpha, layers=4, background=GROUND)), s.want(alpha, 4, front=s.cam.color_buffer),
                     "blended")


def test_more_triangles_than_wavefronts_in_the_cover_grid(oracle):
    """k_peel_cover's grid is capped at kPeelMaxGrid = 8192 workgroups of 4 wavefronts: 32 768 wavefronts, so 70 000
    triangles make every wavefront take a second trip of the triangle loop, some a third."""
    H = W = 64
    assert 70000 > 2 * 8192 * 4
    tri, col, nrm = random_soup(np.random.default_rng(29), 70000, 64, size_px=(0.7, 1.8))
    s = _Scene(oracle, (tri, col, nrm), H, W)
    assert s.covered > 4000 and s.frags.depth >= 8
    f = filler(H, W)
    s.draw(f)
    gw, _ = _check_layers(f, s, 4, "70 000 triangles")
    assert (gw[3] >= 40000).sum() > 100                  # fragments of the second and third trips among the layers


def test_a_row_strip_leaves_the_other_rows_alone(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    frags = peel_ref.fragments(s.tri, s.nrm, s.cam.proj_mat, 200, 173, y0, y1)
    f = filler(200, 173, row_strip=(y0, y1))
    s.draw(f)
    f.synchronize()
    # rows outside the strip: winners and depths that WOULD peel if the pass read them
    f.winner_buffer[:y0] = 0
    f.winner_buffer[y1:] = 5
    f.z_buffer[:y0] = -1.0
    f.z_buffer[y1:] = 0.0
    gw, gz = _check_layers(f, s, 4, "strip", frags=frags, y0=y0, y1=y1)
    assert not gw[:, :y0].any() and not gw[:, y1:].any() and not gz[:, :y0].any() and not gz[:, y1:].any()
    assert (gw[1, y0:y1] >= 0).sum() > 500
    alpha = np.random.default_rng(6).uniform(0, 1, len(s.tri)).astype(np.float32)
    got = host(f.transparency_pass(alpha, layers=3, background=GROUND))
    want = peel_ref.transparency(frags, s.tri, s.col, s.nrm, s.cam.proj_mat, alpha, 3, background=GROUND,
                                 front=s.cam.color_buffer, y0=y0, y1=y1, first_layer=(s.cam.winner, s.cam.z_buffer))
    assert_bit_equal(got, want, "strip: blended")
    assert not got[:y0].any() and not got[y1:].any()


def test_reordered_inputs_go_through_pos_of(oracle):
    tri, col, nrm = random_soup(np.random.default_rng(41), 20000, 256, size_px=(2.0, 30.0))
    s = _Scene(oracle, (tri, col, nrm), 256, 256)
    f = filler(256, 256, presort=True)
    s.draw(f)
    _check_layers(f, s, 5, "presorted")
    assert f._order is not None            # the resident inputs are the tile-coherent copies: the passes went through pos_of
    # alpha is indexed in the caller's order while corners, colours and normals are fetched through pos_of
    alpha = np.random.default_rng(42).uniform(0, 1, len(tri)).astype(np.float32)
    light = oracle.guro_light(LIGHT)
    got = host(f.transparency_pass(alpha, layers=4, light_direction=light, background=GROUND, front="model"))
    assert_bit_equal(got, s.want(alpha, 4, light=light), "presorted: blended")
    s.check_planes(f, "presorted")


# ---- 3. the C entries on hand-built planes -----------------------------------------------------------------------

def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _c_peel_next(lib, winner, z, tri, nrm, P, T=None, pos_of=None, y0=0, y1=None, start=None):
    import torch
    from cython3dmodelrenderer_amd import _capi
    H, W = winner.shape
    T = len(tri) if T is None else T
    y1 = H if y1 is None else y1
    d_tri, d_nrm = (_dev(tri), _dev(nrm)) if T else (None, None)
    d_pos = None if pos_of is None else _dev(pos_of)
    w_out, z_out = (_dev(a) for a in (peel_ref.empty_layer(H, W) if start is None else start))
    keys = torch.empty(lib.crender_atomic_scratch_bytes(H, W) // 8, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_win, d_z = _dev(winner), _dev(z)                 # (named: a temporary's block would be handed to the next one)
    _capi.check(lib.crender_peel_next(d_win.data_ptr(), d_z.data_ptr(), d_tri.data_ptr() if T else None, T,
                                      None if d_pos is None else d_pos.data_ptr(), _capi.f32_16(P),
                                      d_nrm.data_ptr() if T else None, keys.data_ptr(), w_out.data_ptr(), z_out.data_ptr(),
                                      H, W, y0, y1, 0, st), "crender_peel_next")
    return host(w_out), host(z_out)


def test_hand_built_previous_planes_through_the_c_entry(oracle, lib):
    rng = np.random.default_rng(61)
    H, W, T = 64, 61, 400
    tri, col, nrm = random_soup(rng, T, 64, size_px=(5.0, 40.0))
    cam = oracle.OracleFiller(H, W, fov=45.0)
    cam.render_arrays(tri, col, nrm)
    P = cam.proj_mat
    frags = peel_ref.fragments(tri, nrm, P, H, W)
    assert frags.depth >= 6
    w, z = cam.winner.copy(), cam.z_buffer.copy()
    # winners that name no triangle, in columns; depths that are NaN, -0, 0, 1e6, infinite, and any other in rows
    w[:, 0:3], w[:, 3:6], w[:, 6:9], w[:, 9:12], w[:, 12:15] = -1, T, T + 5, 2 ** 31 - 1, -2 ** 31
    w[:, 15:30] = rng.integers(0, T, (H, 15))                        # any triangle, whether it covers the pixel or not
    z[0:4], z[4:8], z[8:12], z[12:16], z[16:20], z[20:24] = np.nan, -0.0, 0.0, 1e6, np.inf, -np.inf
    z[24:40] = rng.uniform(0.6, 1.0, (16, W))
    want = peel_ref.peel_next(frags, w, z)
    got = _c_peel_next(lib, w, z, tri, nrm, P)
    assert_bit_equal(got[0], want[0], "winners")
    assert_bit_equal(got[1], want[1], "z")
    assert (want[0][:, :15] == -1).all() and (want[0][0:4] == -1).all() and (want[0][12:20] == -1).all()
    assert (want[0][20:24, 15:] >= 0).sum() > 100 and (want[0][24:40, 15:] >= 0).sum() > 100
    # d_pos_of: a permutation, some triangles nowhere (they give no fragments and are no valid winners)
    perm = rng.permutation(T).astype(np.uint32)
    pos_of = perm.copy()
    gone = rng.uniform(size=T) < 0.1
    pos_of[gone] = rng.choice(np.uint32([T, T + 7, 2 ** 32 - 1]), int(gone.sum()))
    d_tri, d_nrm = np.zeros_like(tri), np.zeros_like(nrm)
    d_tri[perm], d_nrm[perm] = tri, nrm
    d_tri[perm[gone]], d_nrm[perm[gone]] = np.nan, -1.0                 # never fetched
    under = peel_ref.fragments(tri, nrm, P, H, W, pos_of=pos_of)
    assert len(under) < len(frags)
    want = peel_ref.peel_next(under, w, z, pos_of)
    got = _c_peel_next(lib, w, z, d_tri, d_nrm, P, pos_of=pos_of)
    assert_bit_equal(got[0], want[0], "d_pos_of: winners")
    assert_bit_equal(got[1], want[1], "d_pos_of: z")
    assert (want[0][np.isin(w, np.nonzero(gone)[0])] == -1).all() and not np.isin(want[0], np.nonzero(gone)[0]).any()
    # rows: the others keep what the output planes held
    start = (np.full((H, W), 77, np.int32), np.full((H, W), -5.5, np.float32))
    want = peel_ref.peel_next(frags, w, z, None, 9, 50, out=start)
    got = _c_peel_next(lib, w, z, tri, nrm, P, y0=9, y1=50, start=start)
    assert_bit_equal(got[0], want[0], "rows: winners")
    assert_bit_equal(got[1], want[1], "rows: z")
    assert (got[0][:9] == 77).all() and (got[1][50:] == np.float32(-5.5)).all()


def test_no_triangles(lib):
    import torch
    from cython3dmodelrenderer_amd import _capi
    H, W = 19, 23
    P = np.float32([[2.4, 0, 0, 0], [0, 2.4, 0, 0], [0, 0, 1.0002, 1.0], [0, 0, -0.2, 0]])
    w = np.random.default_rng(1).integers(-2, 3, (H, W)).astype(np.int32)
    z = np.zeros((H, W), np.float32)
    e = np.zeros((0, 3, 3), np.float32)
    got = _c_peel_next(lib, w, z, e, e, P, T=0, start=(np.full((H, W), 7, np.int32), np.full((H, W), 7.0, np.float32)))
    assert (got[0] == -1).all() and (got[1] == np.float32(1e6)).all()
    out, trans = _dev(np.full((H, W, 3), np.nan, np.float32)), _dev(np.full((H, W), np.nan, np.float32))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_win = _dev(w)
    _capi.check(lib.crender_peel_blend(d_win.data_ptr(), None, 0, None, _capi.f32_16(P), None, None, None, None, None,
                                       (C.c_float * 3)(*GROUND), trans.data_ptr(), out.data_ptr(), H, W, 0, H,
                                       _capi.PEEL_FIRST | _capi.PEEL_LAST, st), "crender_peel_blend")
    assert_bit_equal(host(out), np.broadcast_to(np.float32(GROUND), (H, W, 3)), "T = 0: the background")
    assert (host(trans) == 1).all()


# ---- 4. the blend ------------------------------------------------------------------------------------------------

def _alpha(T, seed):
    a = np.random.default_rng(seed).uniform(0, 1, T).astype(np.float32)
    a[::7], a[3::11] = 0.0, 1.0
    return a


@pytest.mark.parametrize("lit", [False, True])
@pytest.mark.parametrize("front", ["plane", "model"])
@pytest.mark.parametrize("scene", ["trex", "soup"])
def test_transparency_pass(oracle, trex256, soup256, filler256, scene, front, lit):
    s, f = (trex256 if scene == "trex" else soup256), filler256
    light = oracle.guro_light(LIGHT) if lit else None
    f.set_fused_illumination(light)
    try:
        s.draw(f)
        alpha = _alpha(len(s.tri), 5)
        n = 5 if scene == "trex" else 6
        # the frame's own colours, lit by the raster kernel or not: the bits the model's shade gives layer 0
        plane = peel_ref.shade(s.cam.winner, s.tri, s.col, s.nrm, s.cam.proj_mat, light)
        assert_bit_equal(host(f.get_color_tensor()), plane, "the frame's colour plane")
        out = f.transparency_pass(alpha, layers=n, light_direction=light, background=GROUND, front=front)
        assert tuple(out.shape) == (256, 256, 3) and out.data_ptr() != f.color_buffer.data_ptr()
        want = s.want(alpha, n, light=light, front=plane if front == "plane" else None)
        assert (want != plane).any() and not np.isnan(want).any()
        assert_bit_equal(host(out), want, f"{scene}, front={front}, lit={lit}")
        # a device tensor is the same; one layer is FIRST and LAST at once
        import torch
        again = f.transparency_pass(torch.from_numpy(alpha).cuda(), layers=1, light_direction=light, background=GROUND, front=front)
        assert_bit_equal(host(again), s.want(alpha, 1, light=light, front=plane if front == "plane" else None), "one layer")
        # alpha = 1: the frame's colour plane bit for bit (over a background of 0, which a cleared frame holds)
        assert_bit_equal(host(f.transparency_pass(1.0, layers=3, light_direction=light, front=front)), plane, "alpha = 1")
        assert_bit_equal(host(f.transparency_pass(0.0, layers=3, background=GROUND, front=front)),
                         np.broadcast_to(np.float32(GROUND), (256, 256, 3)), "alpha = 0")
        assert_bit_equal(host(f.get_color_tensor()), plane, "the colour plane is only read")
        planes_only_read(f, s.cam, scene)
    finally:
        f.set_fused_illumination(None)


def test_a_nan_behind_an_opaque_layer_does_not_spread(soup256, filler256):
    s, f = soup256, filler256
    w, _ = peel_ref.layers(s.frags, 6)
    opaque = np.unique(w[1][w[1] >= 0])
    behind = np.setdiff1d(np.unique(w[2:][w[2:] >= 0]), np.unique(w[:2][w[:2] >= 0]))
    assert len(behind) > 10
    col = s.col.copy()
    col[behind] = np.nan
    alpha = np.full(len(s.tri), 0.5, np.float32)
    alpha[opaque] = 1.0
    f.render_arrays(s.tri, col, s.nrm, clear=True)
    got = host(f.transparency_pass(alpha, layers=6, background=GROUND))
    want = peel_ref.transparency(s.frags, s.tri, col, s.nrm, s.cam.proj_mat, alpha, 6, background=GROUND, front=s.cam.color_buffer)
    assert not np.isnan(want).any()
    assert_bit_equal(got, want, "an opaque second layer")


# ---- 5. the Renderer ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("on_device,device_alpha", [("fused", True), (None, False)])
def test_renderer_with_transparency(oracle, soup256, on_device, device_alpha):
    import torch
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    guro = GuroIllumination(LIGHT)
    alpha = _alpha(len(s.tri), 9)
    f = filler(256, 256)
    given = torch.from_numpy(alpha).cuda() if device_alpha else alpha
    r = Renderer(f, guro, on_device=on_device, transparency=dict(alpha=given, layers=4, background=GROUND))
    light = guro.light_direction
    plane = peel_ref.shade(s.cam.winner, s.tri, s.col, s.nrm, s.cam.proj_mat, light)
    want = s.want(alpha, 4, light=light, front=plane)
    for _ in range(2):                                                    # every frame is drawn from cleared buffers
        got = r.render(s.model)
        if on_device == "fused":
            assert isinstance(got, torch.Tensor)
            got = host(got)
        else:
            assert isinstance(got, np.ndarray)
        assert_bit_equal(got, want, f"Renderer, on_device={on_device}")
