"""The depth-of-field pass on the GPU (csrc/dof.hip's k_dof_blur through AdvancedPixelBufferFiller.depth_of_field, the
C entry and Renderer(depth_of_field=...)), bit for bit against the host model of tests/dof_ref.py evaluated on the oracle's
frames and on hand-built planes (itself pinned in tests/test_dof_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import dof_ref
import phong_ref
from pass_scenes import GOLDEN, Scene, filler, host, lib, soup_fixture, trex_arrays, trex_fixture  # noqa: F401
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)


class _Scene(Scene):
    def want(self, focus, color=None, counts=None, y0=0, y1=None, **kw):
        return dof_ref.dof_blur(self.cam.color_buffer if color is None else color, self.cam.winner, self.cam.z_buffer,
                                len(self.tri), self.cam.proj_mat, focus, y0=y0, y1=y1, counts=counts, **kw)

    def check(self, f, what, focus, counts=None, **kw):
        self.draw(f)
        out = f.depth_of_field(focus, **kw)
        want = self.want(focus, counts=counts, **kw)
        self.assert_changed(want, what)
        assert tuple(out.shape) == (self.H, self.W, 3) and out.data_ptr() != f.color_buffer.data_ptr()
        assert_bit_equal(host(out), want, f"{what}: the result")
        assert_bit_equal(host(f.get_color_tensor()), self.cam.color_buffer, f"{what}: the colour plane is only read")
        self.check_planes(f, what)
        return want


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


@pytest.fixture(scope="module")
def filler256():
    return filler(256, 256)


# ---- 1. T-Rex and the soup at 256 x 256 ------------------------------------------------------------------------

# focus: near the median view depth of the scene's covered pixels (0.987 on T-Rex, 0.847 on the soup); the band: half the
# distance between the quartiles.  (copied, blurred, taps taken) from the host model.  Without a band no covered pixel is
# EXACTLY in focus and the ramp of one pixel reaches every neighbour: nothing is copied.
FOCUS = {"trex": (0.987, 0.0557), "soup": (0.8473, 0.2101)}
PINNED = {
    ("trex", 1, True): (7595, 57941, 496379), ("trex", 8, True): (7591, 57945, 11931068),
    ("trex", 12, True): (7585, 57951, 24012294),
    ("trex", 1, False): (0, 65536, 537587), ("trex", 8, False): (0, 65536, 12359960), ("trex", 12, False): (0, 65536, 24872181),
    ("soup", 1, True): (30744, 34792, 255062), ("soup", 8, True): (21618, 43918, 2723983),
    ("soup", 12, True): (16988, 48548, 4975541),
    ("soup", 1, False): (0, 65536, 522935), ("soup", 8, False): (0, 65536, 9769065), ("soup", 12, False): (0, 65536, 19479352),
}


@pytest.mark.parametrize("band", [True, False])
@pytest.mark.parametrize("R", [1, 8, 12])
@pytest.mark.parametrize("scene", ["trex", "soup"])
def test_scenes_at_every_radius(trex256, soup256, filler256, scene, R, band):
    s = trex256 if scene == "trex" else soup256
    focus, half = FOCUS[scene]
    counts = {}
    s.check(filler256, f"{scene}, max_radius {R}, band={band}", focus, counts=counts, aperture=4.0 * R,
            band=half if band else 0.0, max_radius=R)
    print(f"{scene}, max_radius {R}, band={band}: {counts}")
    assert (counts["copied"], counts["blurred"], counts["taps_taken"]) == PINNED[scene, R, band]
    assert counts["largest_c"] == R and counts["copied"] + counts["blurred"] == 256 * 256
    assert counts["blurred"] >= 0.05 * 256 * 256
    if band:
        assert counts["copied"] >= 0.05 * 256 * 256
    else:
        assert counts["copied"] == 0


def test_aperture_zero_copies_the_frame(soup256, filler256):
    s, f = soup256, filler256
    s.draw(f)
    for R in (1, 12):
        assert_bit_equal(host(f.depth_of_field(0.85, aperture=0.0, max_radius=R)), s.cam.color_buffer, f"aperture 0, max_radius {R}")
    s.check_planes(f, "aperture 0")


# ---- 2. hand-built planes through the C entry ------------------------------------------------------------------

class _Planes:
    """Hand-built planes: view depths around 1 in patches, holes, random colours: what the C entry takes.  No rasterizer
    is involved, so any frame shape goes."""

    def __init__(self, oracle, H, W, seed, T=50, holes=0.15, patch=5):
        rng = np.random.default_rng(seed)
        self.H, self.W, self.T = H, W, T
        self.P = oracle.projection_matrix(45.0, 0.1, 1000.0, max(H, W), max(H, W))    # (any matrix of the shape goes)
        coarse = rng.uniform(0.6, 1.8, ((H + patch - 1) // patch, (W + patch - 1) // patch))
        zv = (np.repeat(np.repeat(coarse, patch, 0), patch, 1)[:H, :W] + rng.uniform(-0.02, 0.02, (H, W))).astype(np.float32)
        self.z = (np.float32(self.P[2, 2]) + np.float32(self.P[3, 2]) / zv).astype(np.float32)
        self.winner = rng.integers(0, T, (H, W)).astype(np.int32)
        self.winner[rng.uniform(size=(H, W)) < holes] = -1
        self.color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)

    def model(self, focus=1.0, counts=None, out=None, **kw):
        for k in ("winner", "z", "color"):
            kw.setdefault(k, getattr(self, k))
        kw.setdefault("T", self.T)
        start = np.full((self.H, self.W, 3), np.nan, np.float32) if out is None else out
        return dof_ref.dof_blur(kw.pop("color"), kw.pop("winner"), kw.pop("z"), kw.pop("T"), self.P, focus, counts=counts,
                                out=start, **kw)

    def device(self, focus=1.0, aperture=4.0, band=0.0, max_radius=8, T=None, y0=0, y1=None, out=None, **planes):
        """The result plane of crender_dof_blur (rows outside y0 .. y1 are `out`'s, NaN without one)."""
        import torch
        from cython3dmodelrenderer_amd import _capi
        L = _capi.load()
        kept = {k: np.ascontiguousarray(planes.get(k, getattr(self, k))) for k in ("winner", "z", "color")}
        dev = {k: torch.from_numpy(v).cuda() for k, v in kept.items()}
        d_out = torch.from_numpy(np.full((self.H, self.W, 3), np.nan, np.float32) if out is None else np.ascontiguousarray(out)).cuda()
        T = self.T if T is None else T
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(L.crender_dof_blur(dev["winner"].data_ptr(), dev["z"].data_ptr(), None, T, None, _capi.f32_16(self.P),
                                       dev["color"].data_ptr(), focus, band, aperture, max_radius, d_out.data_ptr(), self.H,
                                       self.W, y0, self.H if y1 is None else y1, 0, st), "crender_dof_blur")
        got = host(d_out)
        for k in kept:
            assert_bit_equal(host(dev[k]), kept[k], f"{k} is only read")
        return got

    def check(self, what, min_blurred=1, **kw):
        counts = {}
        want = self.model(counts=counts, **kw)
        assert counts["blurred"] >= min_blurred, (what, "the pass changed nothing")
        assert_bit_equal(self.device(**kw), want, what)
        return counts


# 5 x 7, 1 x 40 and 40 x 1: frames smaller than the halo.  33 x 65: one pixel taller and one pixel wider than whole tiles
# of 32.  63 x 31: a partial tile in both directions.
@pytest.mark.parametrize("H,W", [(5, 7), (1, 40), (40, 1), (33, 65), (63, 31)])
def test_frames_that_do_not_fit_the_tiles(oracle, H, W):
    p = _Planes(oracle, H, W, seed=80 + H)
    for R in (1, 12):
        p.check(f"{H} x {W}, max_radius {R}", aperture=3.0 * R, max_radius=R, band=0.05)
        p.check(f"{H} x {W}, max_radius {R}, radii below the clamp", aperture=0.6 * R, max_radius=R)
        if H > 8:
            p.check(f"{H} x {W}, max_radius {R}, rows 3 .. {H - 2}", aperture=3.0 * R, max_radius=R, y0=3, y1=H - 2)


def test_a_frame_of_more_tiles_than_the_grid_holds(oracle):
    """A launch is at most 2048 workgroups, each looping over tiles of 32 x 32: a frame 3 pixels wide and 65 600 tall is
    2050 tiles, so two workgroups make a second trip."""
    p = _Planes(oracle, 65600, 3, seed=91)
    counts = p.check("65600 x 3", aperture=3.0, max_radius=2, band=0.1, min_blurred=1000)
    assert counts["copied"] > 1000
    want = p.model(aperture=3.0, max_radius=2, band=0.1)
    assert (want[65536:].view(np.uint32) != p.color[65536:].view(np.uint32)).any()          # the second trip's rows


def test_tiles_in_focus_beside_tiles_at_the_clamp(oracle):
    """96 x 96: the left tiles exactly in focus (their own reach is 0, they copy), the right ones at the clamp in FRONT of
    them — which spread into the right columns of the sharp tiles (a halo pixel of a sharp tile is blurred by its neighbour
    tile) — and, the other way round, BEHIND them, which do not."""
    p = _Planes(oracle, 96, 96, seed=5, holes=0.0)
    for R in (1, 8, 12):
        for side, depth in (("in front", 0.25), ("behind", 8.0)):
            zv = np.full((96, 96), 1.0, np.float32)
            zv[:, 40:] = depth
            z = (np.float32(p.P[2, 2]) + np.float32(p.P[3, 2]) / zv).astype(np.float32)
            focus = float(dof_ref.view_depth(p.P, z[0, 0]))
            s = dof_ref.coc(p.winner, z, p.T, p.P, focus, 0.0, 40.0, R)[0]
            assert (s[:, :40] == 0).all() and (np.abs(s[:, 40:]) == R).all()
            counts = {}
            want = p.model(focus, counts=counts, z=z, aperture=40.0, max_radius=R)
            changed = (want.view(np.uint32) != p.color.view(np.uint32)).any(2)
            # what is in front reaches R columns into the sharp side (r + 1 - dist > 0 up to dist = R), what is behind none;
            # columns 0 .. 31 are whole tiles, out of every reach for R < 8 and partly within it at 8 and 12
            reach = R if side == "in front" else 0
            assert not changed[:, :40 - reach].any() and changed[:, 40 - reach:].all()
            assert_bit_equal(p.device(focus, z=z, aperture=40.0, max_radius=R), want, f"sharp beside blurred {side}, max_radius {R}")


# ---- 3. special values -----------------------------------------------------------------------------------------

def _assert_equal_up_to_computed_nans(got, want, blurred, what):
    """Bit for bit, but where the model COMPUTED a NaN (a blurred pixel that took a NaN or an infinite colour): there the
    kernel has a NaN as well, whose sign and payload the contract leaves open (the host's and the device's differ).  A
    copied pixel keeps every bit of its NaNs."""
    computed = np.isnan(want) & blurred[..., None]
    assert np.isnan(got[computed]).all(), what
    assert_bit_equal(np.where(computed, np.float32(0), got), np.where(computed, np.float32(0), want), what)


def test_special_values_through_the_c_entry(oracle):
    rng = np.random.default_rng(61)
    H, W = 40, 37
    p = _Planes(oracle, H, W, seed=62, T=30, holes=0.05)
    T = p.T
    z = p.z.copy()
    hit = rng.uniform(size=(H, W)) < 0.12
    z[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf, np.float32(p.P[2, 2]), 1e6]), int(hit.sum()))
    assert (z == np.float32(p.P[2, 2])).any()                        # a division by zero
    winner = p.winner.copy()
    hit = rng.uniform(size=(H, W)) < 0.1
    winner[hit] = rng.choice(np.int32([-2, T, 2 ** 31 - 1, -2 ** 31]), int(hit.sum()))
    color = p.color.copy()
    hit = rng.uniform(size=(H, W)) < 0.05
    color[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf, -0.0]), (int(hit.sum()), 3))
    odd = dict(z=z, winner=winner, color=color)
    seen = dict(computed=False, copied=False)
    for kw in (dict(aperture=3.0, max_radius=1), dict(aperture=20.0, max_radius=8, band=0.1), dict(aperture=40.0, max_radius=12),
               dict(aperture=5.0, max_radius=12, band=0.3), dict(aperture=1e30, max_radius=4), dict(aperture=1e-30, max_radius=4),
               dict(aperture=4.0, max_radius=8, band=1e30), dict(focus=1e-30, aperture=4.0, max_radius=3),
               dict(focus=1e30, aperture=4.0, max_radius=3)):
        blurred = np.zeros((H, W), bool)
        want = p.model(mask=blurred, **odd, **kw)
        seen["computed"] |= bool(np.isnan(want[blurred]).any())
        seen["copied"] |= bool(np.isnan(want[~blurred]).any())
        assert np.isinf(want).any() and blurred.sum() > 50
        _assert_equal_up_to_computed_nans(p.device(**odd, **kw), want, blurred, f"odd values, {kw}")
    assert seen == dict(computed=True, copied=True)                  # NaNs that were taken, and NaNs that were copied
    # aperture 0: the copy keeps -0, the infinities and every NaN
    assert_bit_equal(p.device(aperture=0.0, max_radius=12, **odd), color, "aperture 0 over odd values")
    # T = 0 and a frame that is background only: s = aperture everywhere
    for what, planes in (("T == 0", dict(T=0)), ("background only", dict(winner=np.full((H, W), -1, np.int32)))):
        counts = {}
        want = p.model(counts=counts, aperture=2.5, max_radius=8, z=z, **planes)
        assert counts["covered"] == 0 and counts["blurred"] == H * W and counts["largest_c"] == 2.5
        assert_bit_equal(p.device(aperture=2.5, max_radius=8, z=z, **planes), want, what)


# ---- 4. a row strip --------------------------------------------------------------------------------------------

def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_zero(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    s.draw(f)
    f.synchronize()
    # rows outside the strip: colours, winners and depths that WOULD show if the pass read them
    f.color_buffer[:y0] = 7.5e3
    f.color_buffer[y1:] = -2.25e3
    f.winner_buffer[:y0] = 0
    f.winner_buffer[y1:] = 1
    f.z_buffer[:y0] = float(s.cam.z_buffer[s.cam.winner >= 0].min())
    f.z_buffer[y1:] = float("nan")
    kw = dict(aperture=24.0, band=0.04, max_radius=8)
    focus = 0.987
    got = host(f.depth_of_field(focus, **kw))
    assert not got[:y0].any() and not got[y1:].any()
    counts = {}
    want = s.want(focus, y0=y0, y1=y1, counts=counts, **kw)
    assert counts["blurred"] > 1000 and counts["copied"] > 1000
    assert_bit_equal(got[y0:y1], want[y0:y1], "the strip's rows")
    # the poison works: a pass that looked across the strip's edge would give other colours
    seen = dof_ref.dof_blur(host(f.get_color_tensor()), host(f.get_winner_tensor()), host(f.get_z_tensor()), len(s.tri),
                            s.cam.proj_mat, focus, **kw)
    assert (seen[y0:y1].view(np.uint32) != want[y0:y1].view(np.uint32)).any()
    assert_bit_equal(host(f.get_color_tensor())[y0:y1], s.cam.color_buffer[y0:y1], "the colour plane is only read")


# ---- 5. the filler ---------------------------------------------------------------------------------------------

KW = dict(aperture=20.0, band=0.1, max_radius=6)
SOUP_FOCUS = 0.8473


def test_host_view_edits_reach_the_pass(soup256, filler256):
    s, f = soup256, filler256
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    out = f.depth_of_field(SOUP_FOCUS, **KW)
    want = s.want(SOUP_FOCUS, **KW)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(out), want, "the plain pass")
    assert f.get_color_buffer() is view
    assert_bit_equal(view, s.cam.color_buffer, "the view still shows the frame")
    # an edit of the colour view reaches the pass
    view[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    edited = s.cam.color_buffer.copy()
    edited[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    want_c = s.want(SOUP_FOCUS, color=edited, **KW)
    assert (want_c != want).any()
    assert_bit_equal(host(f.depth_of_field(SOUP_FOCUS, **KW)), want_c, "over edited colours")
    # and one of the z view: a block pushed away from the focus blurs
    s.draw(f)
    zb = f.get_z_buffer()
    block = s.cam.z_buffer.copy()
    block[100:140, 100:140] = np.float32(s.cam.proj_mat[2, 2]) + np.float32(s.cam.proj_mat[3, 2]) / np.float32(3.0)
    zb[:] = block
    want_z = dof_ref.dof_blur(s.cam.color_buffer, s.cam.winner, block, len(s.tri), s.cam.proj_mat, SOUP_FOCUS, **KW)
    assert (want_z != want).any()
    assert_bit_equal(host(f.depth_of_field(SOUP_FOCUS, **KW)), want_z, "under an edited z")
    assert_bit_equal(host(f.get_winner_tensor()), s.cam.winner, "winner")


def test_numpy_torch_and_device_model_inputs_agree(oracle):
    import torch
    from cython3dmodelrenderer_amd import scenes
    from cython3dmodelrenderer_amd.data_structures.device_model import DeviceModel
    from cython3dmodelrenderer_amd.data_structures.model import Model
    from cython3dmodelrenderer_amd.depth_of_field import view_depth
    with np.load(os.path.join(GOLDEN, "trex_mesh.npz")) as z:
        m = Model(z["vertices"], z["faces"])
    scenes.fit_model(m)
    m.set_uniform_color()
    tri, col, nrm = m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles
    s = _Scene(oracle, (tri, col, nrm), 256, 256)
    y, x = np.argwhere(s.cam.winner >= 0)[len(np.argwhere(s.cam.winner >= 0)) // 2]
    kw = dict(aperture=30.0, band=0.03, max_radius=8)
    f = filler(256, 256)                          # numpy
    s.draw(f)
    # the focus on what a pixel shows: from the device's own z, by the module's statement
    focus = float(view_depth(f._P, f.get_z_tensor()[y, x]).item())
    assert focus == float(dof_ref.view_depth(s.cam.proj_mat, s.cam.z_buffer[y, x]))
    want = s.want(focus, **kw)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(f.depth_of_field(focus, **kw)), want, "numpy inputs")
    assert_bit_equal(want[y, x], s.cam.color_buffer[y, x], "the pixel focused on")
    s.check_planes(f, "numpy inputs")
    f = filler(256, 256)                          # caller's device tensors
    f.render_arrays(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (tri, col, nrm)], clear=True)
    assert_bit_equal(host(f.depth_of_field(focus, **kw)), want, "torch inputs")
    f = filler(256, 256)                          # the device-resident model
    f.render_model(DeviceModel(m), clear=True)
    assert_bit_equal(host(f.depth_of_field(focus, **kw)), want, "DeviceModel inputs")
    s.check_planes(f, "DeviceModel inputs")


def test_a_frame_redrawn_after_a_bin_overflow_ends_blurred(oracle):
    """The scene of test_a_frame_redrawn_after_a_bin_overflow_ends_lit: the bin lists are far too small, the frame drops
    fragments and is rendered again when it is settled — which the pass does before it launches."""
    s = _Scene(oracle, random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0), 512, 512)
    kw = dict(aperture=8.0, band=0.2, max_radius=4)
    want = s.want(1.2, **kw)
    assert (want != s.cam.color_buffer).any()
    for more in (dict(), dict(presort=True)):
        f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False, **more)
        s.draw(f)
        need, cap = f.bin_usage()
        assert cap == 500 and need > cap and len(f._pending) == 1     # dropped fragments, nobody has looked yet
        out = f.depth_of_field(1.2, **kw)
        assert not f._pending                                          # grown and redone before the pass
        assert_bit_equal(host(out), want, f"a redone frame, {more}")
        s.check_planes(f, "a redone frame")


# ---- 6. Renderer -----------------------------------------------------------------------------------------------

DOF = dict(focus=SOUP_FOCUS, aperture=20.0, band=0.1, max_radius=6)


@pytest.mark.parametrize("on_device", [None, True, "fused"])
def test_renderer_with_guro_illumination(oracle, soup256, on_device):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    lit = oracle.guro(s.cam.color_buffer.copy(), s.cam.normals_buffer, GURO)
    want = s.want(color=lit, **DOF)
    assert (want != lit).any()
    f = filler(256, 256)
    r = Renderer(f, GuroIllumination(GURO), on_device=on_device, depth_of_field=DOF)
    for _ in range(2):                             # every frame starts from cleared buffers
        out = r.render(s.model)
        assert isinstance(out, np.ndarray) == (on_device is None)
        got = np.array(out) if on_device is None else host(out)
        assert np.array_equal(got, want, equal_nan=True)          # as values: the light leaves -0 on the background
    s.check_planes(f, "after Renderer")
    if on_device == "fused":                       # and by hand, bit for bit: the raster kernel shades, then the pass
        a = filler(256, 256)
        a.set_fused_illumination(GuroIllumination(GURO).light_direction)
        s.draw(a)
        assert_bit_equal(got, host(a.depth_of_field(**DOF)), "the fused light, then depth_of_field")


PHONG_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.25)]
PHONG_KW = dict(ambient=0.15, shininess=16)


def test_renderer_after_the_phong_pass_the_environment_and_the_lines(soup256):
    from cython3dmodelrenderer_amd import environment
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    lit = phong_ref.phong_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.cam.normals_buffer, PHONG_LIGHTS, **PHONG_KW)
    want = s.want(color=lit, **DOF)
    assert (want != lit).any()
    f = filler(256, 256)
    got = host(Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, **PHONG_KW), on_device=True, depth_of_field=DOF).render(s.model))
    assert_bit_equal(got, want, "Renderer(PhongIllumination, depth_of_field=...)")
    # with an environment and lines before it: the passes by hand
    sky = environment.gradient_sky(16)
    wire = dict(width=1.5, color=(250.0, 240.0, 20.0))
    env = dict(reflectivity=0.5, background=True)
    f = filler(256, 256)
    got = host(Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, **PHONG_KW), on_device=True, environment=dict(faces=sky, **env),
                        wireframe=wire, depth_of_field=DOF).render(s.model))
    a = filler(256, 256)
    a.bind_environment(sky)
    s.draw(a)
    a.phong_pass(PHONG_LIGHTS, **PHONG_KW)
    a.environment_pass(**env)
    a.wire_pass(**wire)
    before = host(a.get_color_tensor())
    by_hand = host(a.depth_of_field(**DOF))
    assert (by_hand != before).any() and (before != lit).any()
    assert_bit_equal(got, by_hand, "phong_pass, environment_pass, wire_pass, then depth_of_field")
    assert_bit_equal(by_hand, s.want(color=before, **DOF), "the model over the passes' colours")
    s.check_planes(a, "after the passes")


# ---- 7. errors -------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(soup256):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    f = filler(256, 256, track_winner=False)
    s.draw(f)
    with pytest.raises(ValueError, match="depth_of_field needs the winner plane"):
        f.depth_of_field(1.0)
    f = filler(256, 256)
    with pytest.raises(ValueError, match="depth_of_field: no frame has been rendered"):
        f.depth_of_field(1.0)
    s.draw(f)
    f.render_arrays(s.tri, s.col, s.nrm)           # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.depth_of_field(1.0)
    with pytest.raises(ValueError, match="depth_of_field is not available on a swap chain"):
        filler(64, 64, pipeline=True).depth_of_field(1.0)
    s.draw(f)
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, None):
        with pytest.raises(ValueError, match="focus must be a finite view depth above 0"):
            f.depth_of_field(bad)
    for bad in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="aperture must be a finite number, 0 or above"):
            f.depth_of_field(1.0, aperture=bad)
        with pytest.raises(ValueError, match="band must be a finite number, 0 or above"):
            f.depth_of_field(1.0, band=bad)
    for bad in (0, 13, 8.0, True):
        with pytest.raises(ValueError, match="max_radius must be an int from 1 to 12"):
            f.depth_of_field(1.0, max_radius=bad)
    guro = GuroIllumination(GURO)
    with pytest.raises(ValueError, match="depth_of_field.*together with antialias"):
        Renderer(f, guro, depth_of_field=DOF, antialias={})
    with pytest.raises(ValueError, match="depth_of_field.*together with antialias.*supersample"):
        Renderer(f, guro, depth_of_field=DOF, supersample=2)
    with pytest.raises(ValueError, match=r"\['blades'\] unknown"):
        Renderer(f, guro, depth_of_field=dict(DOF, blades=6))
    with pytest.raises(ValueError, match="object has no depth_of_field"):
        Renderer(object(), guro, depth_of_field=DOF)
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "nothing was written")
    out = f.depth_of_field(**DOF)                  # and works again
    want = s.want(**DOF)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(out), want, "after the errors")
    s.check_planes(f, "after the errors")
