"""Temporal anti-aliasing on the GPU (csrc/temporal.hip's k_taa_resolve through AdvancedPixelBufferFiller.temporal_resolve,
the C entry and Renderer(temporal_aa=...)), bit for bit against the host model of tests/taa_ref.py evaluated on the oracle's
frames and on hand-built planes (itself pinned in tests/test_taa_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_ref
import taa_ref
from pass_scenes import GOLDEN, Scene, filler, host, lib, soup_fixture, trex_arrays, trex_fixture  # noqa: F401
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)
MODES = {"static": (False, False), "velocity": (True, False), "dilated": (True, True)}       # (a velocity plane, the z plane)


def _noise(shape, seed, lo=0.0, hi=255.0):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32)


class _Scene(Scene):
    def previous(self, angles):
        return motion_ref.rotated(self.tri, angles)

    def vectors(self, prev, **kw):
        return motion_ref.motion_vectors(self.cam.winner, self.tri, self.cam.proj_mat, prev, **kw)

    def history(self, seed=7):
        """Half the frame, half noise: a history that the box clamps in places and leaves alone in others."""
        return (self.cam.color_buffer * np.float32(0.5) + _noise(self.cam.color_buffer.shape, seed) * np.float32(0.5)).astype(np.float32)

    def want(self, history, velocity=None, dilate=True, clamp=True, blend=0.1, color=None, z=None, **kw):
        z = (self.cam.z_buffer if z is None else z) if dilate and velocity is not None else None
        return taa_ref.resolve(self.cam.color_buffer if color is None else color, history, velocity, z, blend,
                               flags=0 if clamp else taa_ref.NO_CLAMP, **kw)


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


@pytest.fixture(scope="module")
def filler256():
    return filler(256, 256)


# ---- 1. T-Rex and the soup at 256 x 256 ------------------------------------------------------------------------

POSES = {"trex fast": ("trex", (0, 10, 0)), "trex slow": ("trex", (0, 2, 0)), "soup z": ("soup", (0, 0, 5)),
         "soup y": ("soup", (0, 3, 0))}                 # test_motion_gpu.py's


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("pose", list(POSES))
def test_scenes_in_every_instance(trex256, soup256, filler256, pose, mode):
    scene, angles = POSES[pose]
    s, f = (trex256 if scene == "trex" else soup256), filler256
    prev = s.previous(angles)
    hist = s.history()
    moving, dilate = MODES[mode]
    v = s.vectors(prev) if moving else None
    s.draw(f)
    for clamp in (True, False):
        for blend in (0.1, 0.5):
            what = f"{pose}, {mode}, clamp {clamp}, blend {blend}"
            counts = {}
            want = s.want(hist, v, dilate, clamp, blend, counts=counts)
            out = f.temporal_resolve(hist, prev if moving else None, blend=blend, dilate=dilate, clamp=clamp)
            assert tuple(out.shape) == (s.H, s.W, 3) and out.data_ptr() != f.color_buffer.data_ptr()
            assert_bit_equal(host(out), want, what)
            assert (want != s.cam.color_buffer).any() and (counts["four"] > 1000) == moving, (what, counts)
    if moving:       # the same from the velocity plane, and the dilation is not the plain velocity
        assert_bit_equal(host(f.temporal_resolve(hist, velocity=v, dilate=dilate)), s.want(hist, v, dilate), f"{pose}, {mode}: velocity=")
        assert (s.want(hist, v, True) != s.want(hist, v, False)).any()
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, f"{pose}, {mode}: the colour plane is only read")
    s.check_planes(f, f"{pose}, {mode}")


# ---- 2. hand-built planes through the C entry ------------------------------------------------------------------

class _Planes:
    """Hand-built planes: random colours and history, depths in patches, velocities in patches of their own (a third of them
    still): what the C entry takes.  No rasterizer is involved, so any frame shape goes."""

    def __init__(self, H, W, seed, patch=5, speed=6.0):
        rng = np.random.default_rng(seed)
        self.H, self.W = H, W
        self.color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
        self.history = rng.uniform(-50, 300, (H, W, 3)).astype(np.float32)
        coarse = rng.integers(1, 6, ((H + patch - 1) // patch, (W + patch - 1) // patch)).astype(np.float32) / np.float32(8)
        self.z = np.ascontiguousarray(np.repeat(np.repeat(coarse, patch, 0), patch, 1)[:H, :W])     # equal depths abound: ties
        big = 7
        vc = rng.uniform(-speed, speed, ((H + big - 1) // big, (W + big - 1) // big, 2))
        vc[rng.uniform(size=vc.shape[:2]) < 0.3] = 0
        self.velocity = (np.repeat(np.repeat(vc, big, 0), big, 1)[:H, :W] + rng.uniform(-0.3, 0.3, (H, W, 2))).astype(np.float32)

    def planes(self, mode, **kw):
        moving, dilate = MODES[mode]
        return (kw.get("color", self.color), kw.get("history", self.history), kw.get("velocity", self.velocity) if moving else None,
                kw.get("z", self.z) if dilate else None)

    def model(self, mode, blend=0.1, flags=0, y0=0, y1=None, counts=None, **kw):
        start = np.full((self.H, self.W, 3), np.nan, np.float32)
        return taa_ref.resolve(*self.planes(mode, **kw), blend, y0, y1, flags, out=start, counts=counts)

    def device(self, mode, blend=0.1, flags=0, y0=0, y1=None, **kw):
        """The result plane of crender_taa_resolve (rows outside y0 .. y1 are NaN)."""
        import torch
        from cython3dmodelrenderer_amd import _capi
        L = _capi.load()
        kept = [None if p is None else np.ascontiguousarray(p) for p in self.planes(mode, **kw)]
        dev = [None if p is None else torch.from_numpy(p).cuda() for p in kept]
        d_out = torch.from_numpy(np.full((self.H, self.W, 3), np.nan, np.float32)).cuda()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(L.crender_taa_resolve(*[None if d is None else d.data_ptr() for d in dev], blend, d_out.data_ptr(), self.H,
                                          self.W, y0, self.H if y1 is None else y1, flags, st), "crender_taa_resolve")
        got = host(d_out)
        for k, d in zip(kept, dev):
            if k is not None:
                assert_bit_equal(host(d).view(np.uint32), k.view(np.uint32), "an input plane is only read")
        return got

    def check(self, what, mode, min_four=0, **kw):
        counts = {}
        want = self.model(mode, counts=counts, **kw)
        assert counts["four"] >= min_four, (what, counts)
        taa_ref.assert_matches(self.device(mode, **kw), want, what)
        return counts


# 5 x 7, 1 x 40 and 40 x 1: frames smaller than a tile, one of them a single row, one a single column.  33 x 65: one pixel
# taller and one pixel wider than whole tiles of 32.  63 x 31: a partial tile in both directions.
@pytest.mark.parametrize("H,W", [(5, 7), (1, 40), (40, 1), (33, 65), (63, 31)])
def test_frames_that_do_not_fit_the_tiles(H, W):
    p = _Planes(H, W, seed=80 + H)
    if H == 1 or W == 1:
        p.velocity[..., 1 if H == 1 else 0] = 0          # along the line, or every previous position leaves the frame
    for mode in MODES:
        for flags in (0, 1):
            for blend in (0.1, 0.5, 1.0):
                p.check(f"{H} x {W}, {mode}, flags {flags}, blend {blend}", mode, flags=flags, blend=blend,
                        min_four=1 if MODES[mode][0] and blend < 1 and H * W > 40 else 0)
            if H > 8:
                p.check(f"{H} x {W}, {mode}, flags {flags}, rows 3 .. {H - 2}", mode, flags=flags, y0=3, y1=H - 2)
    assert_bit_equal(p.device("dilated", blend=1.0)[...], p.color, "blend = 1 copies the bits")


def test_a_frame_of_more_tiles_than_the_grid_holds():
    """A launch is at most 2048 workgroups, each looping over tiles of 32 x 32: a frame 3 pixels wide and 65 600 tall is
    2050 tiles, so two workgroups make a second trip."""
    p = _Planes(65600, 3, seed=91, speed=2.0)
    for mode, flags in (("dilated", 0), ("static", 1)):
        want = p.model(mode, flags=flags)
        assert (want[65536:] != p.color[65536:]).any()          # the second trip's rows
        taa_ref.assert_matches(p.device(mode, flags=flags), want, f"65600 x 3, {mode}")


def _still(H=96, W=96, seed=5):
    p = _Planes(H, W, seed=seed)
    p.velocity = np.zeros((H, W, 2), np.float32)
    return p


def test_whole_pixels_halves_and_the_frames_boundaries():
    p = _still()
    H, W = p.H, p.W
    # whole pixels everywhere: one texel a pixel, by the wavefront's scalar branch; then one pixel with a fraction among them
    for vx, vy in ((3, 0), (0, -2), (-5, 7), (0, 0)):
        v = p.velocity.copy()
        v[:] = np.float32([vx, vy])
        for mode in ("velocity", "dilated"):
            c = p.check(f"whole pixels {(vx, vy)}, {mode}", mode, velocity=v, blend=0.25)
            assert c["four"] == 0 and c["kept"] == H * W - (H - abs(vy)) * (W - abs(vx))
        v[40, 40] = (vx + 0.25, vy)
        assert p.check(f"one fraction among {(vx, vy)}", "velocity", velocity=v, blend=0.25)["four"] == 1
    # exact halves, in x, in y and in both
    for vx, vy in ((0.5, 0), (0, 0.5), (-2.5, 1.5), (1.5, -0.5)):
        v = p.velocity.copy()
        v[:] = np.float32([vx, vy])
        v[::3, ::2] = 0
        for flags in (0, 1):
            assert p.check(f"halves {(vx, vy)}, flags {flags}", "dilated", velocity=v, flags=flags, min_four=3000)["four"] < H * W
    # leaving each side, and landing exactly on the boundary texels: px = 0, W - 1, py = 0, H - 1 count, half a pixel further does not
    v = p.velocity.copy()
    ys, xs = np.mgrid[0:H, 0:W]
    v[:, :8, 0] = (xs[:, :8] + (ys[:, :8] % 3 - 1) * 0.5).astype(np.float32)           # px = 0.5, 0, -0.5 by the row
    v[:, -8:, 0] = (xs[:, -8:] - (W - 1) + (ys[:, -8:] % 3 - 1) * 0.5).astype(np.float32)      # px = W - 0.5, W - 1, W - 1.5
    v[:8, 8:-8, 1] = (ys[:8, 8:-8] + (xs[:8, 8:-8] % 3 - 1) * 0.5).astype(np.float32)
    v[-8:, 8:-8, 1] = (ys[-8:, 8:-8] - (H - 1) + (xs[-8:, 8:-8] % 3 - 1) * 0.5).astype(np.float32)
    for mode in ("velocity", "dilated"):
        c = p.check(f"the frame's boundaries, {mode}", mode, velocity=v, blend=0.25, flags=1)
        assert c["kept"] > 300 and c["four"] > 300
    got = p.device("velocity", velocity=v, blend=0.25, flags=1)
    keep = np.float32(0.75)
    assert_bit_equal(got[1, 3], p.color[1, 3] + (p.history[1, 0] - p.color[1, 3]) * keep, "px = 0 reads column 0")
    assert_bit_equal(got[2, 3], p.color[2, 3], "px = -0.5 keeps the colour")
    assert_bit_equal(got[1, W - 3], p.color[1, W - 3] + (p.history[1, W - 1] - p.color[1, W - 3]) * keep, "px = W - 1 reads the last column")
    assert_bit_equal(got[0, W - 3], p.color[0, W - 3], "px = W - 0.5 keeps the colour")
    # the same boundaries of a strip, whose first and last rows are the edge
    for mode in ("velocity", "dilated"):
        v = p.velocity.copy()
        v[20:28, :, 1] = (ys[20:28] - 20 + (xs[20:28] % 3 - 1) * 0.5).astype(np.float32)       # py = 19.5, 20, 20.5
        v[60:70, :, 1] = (ys[60:70] - 69 + (xs[60:70] % 3 - 1) * 0.5).astype(np.float32)       # py = 68.5, 69, 69.5
        c = p.check(f"the strip's boundaries, {mode}", mode, velocity=v, y0=20, y1=70, flags=1)
        assert c["kept"] > 300 and c["four"] > 300


def test_lone_fast_pixels_on_the_tile_seams_with_depth_ties_across_them():
    p = _still()
    p.z[:] = np.float32(0.5)
    v = p.velocity.copy()
    fast = [(31, 31), (31, 32), (32, 31), (32, 32), (31, 64), (64, 31), (63, 63), (64, 64), (10, 31), (10, 32), (31, 10), (32, 10)]
    for k, (y, x) in enumerate(fast):
        v[y, x] = (1.25 + 0.5 * k, -(0.5 + 0.5 * k))   # (every previous position is on the frame, none on a whole pixel)
        p.z[y, x] = np.float32(0.25)                    # equal among them: around a seam's corner four pixels tie
    sy, sx = taa_ref.dilated_source(p.z)
    assert (sy[32, 32], sx[32, 32]) == (32, 32) and (sy[31, 31], sx[31, 31]) == (31, 31) and (sy[33, 33], sx[33, 33]) == (32, 32)
    assert (sy[33, 32], sx[33, 32]) == (32, 31) and (sy[31, 33], sx[31, 33]) == (31, 32)      # the first of two equal ones
    assert (sy[32, 33], sx[32, 33]) == (31, 32) and (sy[30, 30], sx[30, 30]) == (31, 31)
    for flags in (0, 1):
        c = p.check(f"fast pixels on the seams, flags {flags}", "dilated", velocity=v, flags=flags)
        assert c["four"] >= 9 * 4
        plain = p.check(f"the same without the z plane, flags {flags}", "velocity", velocity=v, flags=flags)
        assert plain["four"] == len(fast)
    # a strip whose edge runs along the seam does not see the fast pixels across it
    c = p.check("a strip from the seam on", "dilated", velocity=v, y0=32, y1=96)
    sy, _ = taa_ref.dilated_source(p.z, 32, 96)
    assert sy.min() == 32


def test_special_values_through_the_c_entry():
    rng = np.random.default_rng(61)
    H, W = 40, 37
    p = _Planes(H, W, seed=62)
    odd = np.float32([np.nan, np.inf, -np.inf, 1e30, -1e30])
    planes = {}
    for name, share in (("velocity", 0.15), ("z", 0.12), ("color", 0.06), ("history", 0.06)):
        a = getattr(p, name).copy()
        hit = rng.uniform(size=(H, W)) < share
        a[hit] = rng.choice(odd, (int(hit.sum()),) + a.shape[2:])
        planes[name] = a
    planes["color"][5, 5].view(np.uint32)[:] = [0x7FC00123, 0xFFC00001, 0x80000000]       # NaN payloads and -0 ...
    planes["velocity"][5, 5] = (100, 0)                                                   # ... in a pixel that is kept
    seen = dict(nan=False, inf=False)
    for mode in MODES:
        for flags in (0, 1):
            for kw in (dict(), dict(y0=3, y1=H - 2)):
                want = p.model(mode, flags=flags, blend=0.25, **planes, **kw)
                seen["nan"] |= bool(np.isnan(want[3:H - 2]).any())
                seen["inf"] |= bool(np.isinf(want[3:H - 2]).any())
                got = p.device(mode, flags=flags, blend=0.25, **planes, **kw)
                taa_ref.assert_matches(got, want, f"odd values, {mode}, flags {flags}, {kw}")
                if mode == "velocity":
                    assert_bit_equal(got[5, 5], planes["color"][5, 5], "a kept pixel keeps every bit")
    assert seen == dict(nan=True, inf=True)
    # each plane's odd values alone, so that a finite result cannot hide behind another plane's NaN
    for name in planes:
        taa_ref.assert_matches(p.device("dilated", blend=0.25, **{name: planes[name]}),
                               p.model("dilated", blend=0.25, **{name: planes[name]}), f"odd {name} alone")
    assert_bit_equal(p.device("dilated", blend=1.0, **planes), planes["color"], "blend = 1 copies the bits")


# ---- 3. a row strip, and the filler ----------------------------------------------------------------------------

def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_zero(oracle):
    import torch
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    prev = s.previous((0, 10, 0))
    f = filler(200, 173, row_strip=(y0, y1))
    s.draw(f)
    f.synchronize()
    want_v = s.vectors(prev, y0=y0, y1=y1)
    hist = s.history()
    # rows outside the strip: colours, depths, velocities and a history that WOULD show if the pass read them
    f.color_buffer[:y0] = 7.5e3
    f.color_buffer[y1:] = -2.25e3
    f.z_buffer[:y0] = -1.0
    f.z_buffer[y1:] = float("-inf")
    poisoned = torch.from_numpy(want_v).cuda()
    poisoned[:y0] = torch.tensor([0.0, 30.0], device="cuda")
    poisoned[y1:] = torch.tensor([-30.0, -30.0], device="cuda")
    hist[:y0], hist[y1:] = 1e4, -1e4
    want = s.want(hist, want_v, y0=y0, y1=y1, blend=0.25)
    for given in (dict(velocity=poisoned), dict(previous_vertices=prev)):
        got = host(f.temporal_resolve(hist, blend=0.25, **given))
        assert not got[:y0].any() and not got[y1:].any()
        assert_bit_equal(got[y0:y1], want[y0:y1], f"the strip's rows, {list(given)}")
    # the poison works: a pass that looked across the strip's edge would give other colours
    seen = taa_ref.resolve(host(f.get_color_tensor()), hist, host(poisoned), host(f.get_z_tensor()), 0.25)
    assert (seen[y0:y1].view(np.uint32) != want[y0:y1].view(np.uint32)).any()
    for mode in ("static", "velocity"):
        moving, _ = MODES[mode]
        got = host(f.temporal_resolve(hist, velocity=poisoned if moving else None, dilate=False, clamp=False, blend=0.5))
        assert_bit_equal(got[y0:y1], s.want(hist, want_v if moving else None, False, False, 0.5, y0=y0, y1=y1)[y0:y1], f"the strip, {mode}")
    none = host(f.temporal_resolve(None))
    assert not none[:y0].any() and not none[y1:].any()
    assert_bit_equal(none[y0:y1], s.cam.color_buffer[y0:y1], "no history: the strip's rows, copied")
    assert_bit_equal(host(f.get_color_tensor())[y0:y1], s.cam.color_buffer[y0:y1], "the colour plane is only read")


ANGLES = (0, 0, 5)


def test_host_view_edits_reach_the_pass(soup256, filler256):
    s, f = soup256, filler256
    prev, hist = s.previous(ANGLES), s.history()
    v = s.vectors(prev)
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    want = s.want(hist, v, blend=0.3)
    assert_bit_equal(host(f.temporal_resolve(hist, prev, blend=0.3)), want, "the plain pass")
    assert f.get_color_buffer() is view
    assert_bit_equal(view, s.cam.color_buffer, "the view still shows the frame")
    # an edit of the colour view reaches the pass: the colour, and the box around it
    view[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    edited = s.cam.color_buffer.copy()
    edited[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    want_c = s.want(hist, v, blend=0.3, color=edited)
    assert (want_c != want).any()
    assert_bit_equal(host(f.temporal_resolve(hist, prev, blend=0.3)), want_c, "over edited colours")
    # and one of the z view: a block pulled to the front gives its velocity to the pixels around it
    s.draw(f)
    zb = f.get_z_buffer()
    block = s.cam.z_buffer.copy()
    block[100:140, 100:140] = np.float32(-1.0)
    zb[:] = block
    want_z = s.want(hist, v, blend=0.3, z=block)
    assert (want_z != want).any()
    assert_bit_equal(host(f.temporal_resolve(hist, prev, blend=0.3)), want_z, "under an edited z")
    assert_bit_equal(host(f.get_winner_tensor()), s.cam.winner, "winner")


def test_numpy_torch_and_device_model_inputs_agree(oracle):
    import torch
    from cython3dmodelrenderer_amd import scenes
    from cython3dmodelrenderer_amd.data_structures.device_model import DeviceModel
    from cython3dmodelrenderer_amd.data_structures.model import Model
    with np.load(os.path.join(GOLDEN, "trex_mesh.npz")) as z:
        m = Model(z["vertices"], z["faces"])
    scenes.fit_model(m)
    m.set_uniform_color()
    tri, col, nrm = m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles
    s = _Scene(oracle, (tri, col, nrm), 256, 256)
    prev, hist = s.previous((0, 8, 0)), s.history()
    want = s.want(hist, s.vectors(prev), blend=0.2)
    assert (want != s.cam.color_buffer).any()
    f = filler(256, 256)                          # numpy
    s.draw(f)
    assert_bit_equal(host(f.temporal_resolve(hist, prev, blend=0.2)), want, "numpy inputs")
    s.check_planes(f, "numpy inputs")
    f = filler(256, 256)                          # caller's device tensors
    f.render_arrays(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (tri, col, nrm)], clear=True)
    d_prev, d_hist = torch.from_numpy(prev).cuda(), torch.from_numpy(hist).cuda()
    assert_bit_equal(host(f.temporal_resolve(d_hist, d_prev, blend=0.2)), want, "torch inputs")
    assert_bit_equal(host(d_hist), hist, "the history is only read")
    f = filler(256, 256)                          # the device-resident model
    dm = DeviceModel(m)
    f.render_model(dm, clear=True)
    assert_bit_equal(host(f.temporal_resolve(d_hist, d_prev, blend=0.2)), want, "DeviceModel inputs")
    s.check_planes(f, "DeviceModel inputs")
    # sheared on device tensors is the numpy form, bit for bit
    for jx, jy in taa_ref.jitter_offsets(8):
        k = taa_ref.view_shear(f._P, 256, 256, jx, jy)
        got = taa_ref.sheared(dm._vertices_by_triangles, *k)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.data_ptr() != dm._vertices_by_triangles.data_ptr()
        assert_bit_equal(host(got), taa_ref.sheared(np.ascontiguousarray(tri), *k), f"sheared by {(jx, jy)}")
    assert_bit_equal(host(dm._vertices_by_triangles), tri, "the model's vertices are only read")


def test_a_frame_redrawn_after_a_bin_overflow_ends_resolved(oracle):
    """The scene of test_a_frame_redrawn_after_a_bin_overflow_ends_lit: the bin lists are far too small, the frame drops
    fragments and is rendered again when it is settled — which the pass does before it launches."""
    s = _Scene(oracle, random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0), 512, 512)
    prev, hist = s.previous((0, 0, 2)), s.history()
    want = s.want(hist, s.vectors(prev), blend=0.3)
    assert (want != s.cam.color_buffer).any()
    for more in (dict(), dict(presort=True)):
        f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False, **more)
        s.draw(f)
        need, cap = f.bin_usage()
        assert cap == 500 and need > cap and len(f._pending) == 1     # dropped fragments, nobody has looked yet
        out = f.temporal_resolve(hist, prev, blend=0.3)
        assert not f._pending                                          # grown and redone before the pass
        assert_bit_equal(host(out), want, f"a redone frame, {more}")
        s.draw(f)
        assert_bit_equal(host(f.temporal_resolve(hist, blend=0.3)), s.want(hist, blend=0.3), f"a static view, {more}")
        s.check_planes(f, "a redone frame")


# ---- 4. Renderer -----------------------------------------------------------------------------------------------

class _Turning:
    """The soup as a model whose vertex array is replaced by the next pose between two frames."""

    def __init__(self, s, n=4):
        self.poses = [s.previous((0, 0, 2 * (n - 1 - i))) for i in range(n - 1)] + [s.tri]
        self._vertices_by_triangles, self._colors_by_triangles, self._normals_by_triangles = self.poses[0], s.col, s.nrm


def _image(a):
    return np.array(a) if isinstance(a, np.ndarray) else host(a)


def _by_hand(b, poses, n, history, light, cycle=8, floor=0.1, **kw):
    """Frame n of the sequence on the filler `b`, the passes made by hand: the sheared pose drawn, `light(b)`, the resolve."""
    k = taa_ref.view_shear(b._P, b.h, b.w, *taa_ref.jitter_offsets(cycle)[n % cycle])
    light(b, taa_ref.sheared(poses[n], *k))
    if n == 0:
        return b.temporal_resolve(None)
    return b.temporal_resolve(history, previous_vertices=taa_ref.sheared(poses[n - 1], *k), blend=max(floor, 1.0 / (n + 1)), **kw)


@pytest.mark.parametrize("on_device", [None, True, "fused"])
def test_renderer_with_guro_illumination(soup256, on_device):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    guro = GuroIllumination(GURO)

    def light(b, tri):
        if on_device == "fused":
            guro.fuse_into(b)
            b.render_arrays(tri, s.col, s.nrm, clear=True)
        else:
            b.set_fused_illumination(None)
            b.render_arrays(tri, s.col, s.nrm, clear=True)
            assert guro.draw_illumination_device(b)
    f, b = filler(256, 256), filler(256, 256)
    r = Renderer(f, guro, on_device=on_device, temporal_aa=dict(blend=0.1))
    m = _Turning(s)
    history, images = None, []
    for n in range(4):
        m._vertices_by_triangles = m.poses[n]
        got = r.render(m)
        assert isinstance(got, np.ndarray) == (on_device is None)
        images.append(_image(got))
        history = _by_hand(b, m.poses, n, history, light)
        assert_bit_equal(images[n], host(history), f"on_device={on_device!r}: frame {n}")
    # the first call is the jittered frame, copied; the later ones are neither their frame nor the one before
    k = taa_ref.view_shear(b._P, 256, 256, *taa_ref.jitter_offsets(8)[0])
    light(b, taa_ref.sheared(m.poses[0], *k))
    assert_bit_equal(images[0], host(b.get_color_tensor()), "the first call")
    assert (images[1] != images[0]).any() and (images[3] != images[2]).any()
    # reset_motion(): frame 0 again
    r.reset_motion()
    m._vertices_by_triangles = m.poses[0]
    assert_bit_equal(_image(r.render(m)), images[0], "after reset_motion()")
    s_planes = host(f.get_winner_tensor())
    assert (s_planes >= 0).sum() > 10000


PHONG_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.25)]
PHONG_KW = dict(ambient=0.15, shininess=16)


def test_renderer_after_the_phong_pass_and_with_bloom_after_it(soup256):
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    glow = dict(threshold=150.0, radius=4)
    opts = dict(blend=0.25, jitter=3, dilate=False)

    def light(b, tri):
        b.set_fused_illumination(None)
        b.render_arrays(tri, s.col, s.nrm, clear=True)
        b.phong_pass(PHONG_LIGHTS, **PHONG_KW)
    f, b = filler(256, 256), filler(256, 256)
    r = Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, **PHONG_KW), on_device=True, temporal_aa=opts, bloom=glow)
    m = _Turning(s)
    history = None
    for n in range(4):
        m._vertices_by_triangles = m.poses[n]
        got = _image(r.render(m))
        history = _by_hand(b, m.poses, n, history, light, cycle=3, floor=0.25, dilate=False)
        by_hand = host(b.bloom(source=history, **glow))
        assert (by_hand != host(history)).any()
        assert_bit_equal(got, by_hand, f"phong_pass, temporal_resolve, then bloom: frame {n}")


# ---- 5. errors -------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(soup256):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    prev, hist = s.previous(ANGLES), s.history()
    f = filler(256, 256, track_winner=False)
    s.draw(f)
    with pytest.raises(ValueError, match="temporal_resolve needs the winner plane"):
        f.temporal_resolve(hist)
    f = filler(256, 256)
    with pytest.raises(ValueError, match="temporal_resolve: no frame has been rendered"):
        f.temporal_resolve(hist)
    s.draw(f)
    f.render_arrays(s.tri, s.col, s.nrm)           # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.temporal_resolve(hist)
    with pytest.raises(ValueError, match="temporal_resolve is not available on a swap chain"):
        filler(64, 64, pipeline=True).temporal_resolve(hist)
    s.draw(f)
    T = len(s.tri)
    with pytest.raises(ValueError, match=f"previous_vertices holds {T - 2} triangles, the last frame drew {T}"):
        f.temporal_resolve(hist, prev[2:])
    with pytest.raises(ValueError, match="at most one of previous_vertices and velocity"):
        f.temporal_resolve(hist, prev, velocity=np.zeros((256, 256, 2), np.float32))
    with pytest.raises(ValueError, match="velocity must be float32"):
        f.temporal_resolve(hist, velocity=np.zeros((256, 255, 2), np.float32))
    with pytest.raises(ValueError, match="history must be None or float32"):
        f.temporal_resolve(hist[:, :255])
    for bad in (0.0, -1.0, 1.5, float("nan"), float("inf"), None, True):
        with pytest.raises(ValueError, match="blend must be a number above 0 and at most 1"):
            f.temporal_resolve(hist, blend=bad)
    for bad in (0, None, "no"):
        with pytest.raises(ValueError, match="dilate must be a bool"):
            f.temporal_resolve(hist, prev, dilate=bad)
        with pytest.raises(ValueError, match="clamp must be a bool"):
            f.temporal_resolve(hist, clamp=bad)
    guro = GuroIllumination(GURO)
    for other in (dict(antialias={}), dict(depth_of_field=dict(focus=1.0)), dict(motion_blur={}), dict(supersample=2),
                  dict(transparency=dict(alpha=0.5))):
        with pytest.raises(ValueError, match="temporal_aa.*together with antialias"):
            Renderer(f, guro, temporal_aa={}, **other)
    with pytest.raises(ValueError, match=r"\['frames'\] unknown"):
        Renderer(f, guro, temporal_aa=dict(frames=1))
    with pytest.raises(ValueError, match="jitter must be an int from 0 to 64"):
        Renderer(f, guro, temporal_aa=dict(jitter=65))
    with pytest.raises(ValueError, match="object has no temporal_resolve"):
        Renderer(object(), guro, temporal_aa={})
    # the C entry refuses an aliased result before it launches
    import torch
    from cython3dmodelrenderer_amd import _capi
    d_hist = torch.from_numpy(hist).cuda()
    before = host(d_hist)
    rc = _capi.load().crender_taa_resolve(f.color_buffer.data_ptr(), d_hist.data_ptr(), None, None, 0.5, d_hist.data_ptr(), 256, 256,
                                          0, 256, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _capi.EINVAL and b"d_out is d_color or d_history" in _capi.load().crender_last_error()
    assert_bit_equal(host(d_hist), before, "a refused call writes nothing")
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "nothing was written")
    out = f.temporal_resolve(hist, prev, blend=0.3)                # and works again
    want = s.want(hist, s.vectors(prev), blend=0.3)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(out), want, "after the errors")
    s.check_planes(f, "after the errors")
