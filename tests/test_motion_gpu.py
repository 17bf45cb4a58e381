"""The motion passes on the GPU (csrc/motion.hip's k_motion_vectors and k_motion_blur through
AdvancedPixelBufferFiller.motion_vectors / motion_blur, the C entries and Renderer(motion_blur=...)), bit for bit against the
host model of tests/motion_ref.py evaluated on the oracle's frames and on hand-built planes (itself pinned in
tests/test_motion_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_ref
import phong_ref
from pass_scenes import GOLDEN, Scene, filler, host, lib, soup_fixture, trex_arrays, trex_fixture  # noqa: F401
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)


class _Scene(Scene):
    def previous(self, angles):
        return motion_ref.rotated(self.tri, angles)

    def vectors(self, prev, **kw):
        return motion_ref.motion_vectors(self.cam.winner, self.tri, self.cam.proj_mat, prev, **kw)

    def want(self, velocity, color=None, **kw):
        return motion_ref.motion_blur(self.cam.color_buffer if color is None else color, self.cam.winner, self.cam.z_buffer,
                                      len(self.tri), self.cam.proj_mat, velocity, **kw)

    def check(self, f, what, prev, counts=None, exposure=1.0, **kw):
        self.draw(f)
        v = f.motion_vectors(prev, exposure=exposure)
        want_v = self.vectors(prev, exposure=exposure)
        assert tuple(v.shape) == (self.H, self.W, 2)
        assert_bit_equal(host(v), want_v, f"{what}: the velocity plane")
        out = f.motion_blur(prev, exposure=exposure, **kw)
        want = self.want(want_v, counts=counts, **kw)
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

# The previous pose: the scene rotated about the float32 mean of its corners.  Half lengths up to 8.75 px on T-Rex at 10
# degrees about y (the clamp at max_radius 8) and 1.75 px at 2 degrees (the slow scene: 64 % of the covered pixels at or under
# 1/2); up to 8.15 px on the soup at 5 degrees about z and 21.7 px at 3 degrees about y (the clamp everywhere).
# (moving, tiles that copy, copied, blurred, taps taken) from the host model.  With max_radius 1 and 2 taps every offset
# is rint(+-D / 2) with |D| <= 1, which is 0: nothing is blurred, a consequence of the rule that is pinned like the others.
POSES = {"trex fast": ("trex", (0, 10, 0)), "trex slow": ("trex", (0, 2, 0)), "soup z": ("soup", (0, 0, 5)),
         "soup y": ("soup", (0, 3, 0))}
PINNED = {
    ("trex fast", 1, 2): (14364, 35, 65536, 0, 0), ("trex fast", 1, 15): (14364, 35, 53655, 11881, 88158),
    ("trex fast", 1, 32): (14364, 35, 53655, 11881, 179311), ("trex fast", 8, 2): (14364, 29, 57009, 8527, 15371),
    ("trex fast", 8, 15): (14364, 29, 52067, 13469, 90404), ("trex fast", 8, 32): (14364, 29, 52070, 13466, 191207),
    ("trex fast", 12, 2): (14364, 27, 58256, 7280, 12999), ("trex fast", 12, 15): (14364, 27, 52038, 13498, 85881),
    ("trex fast", 12, 32): (14364, 27, 52028, 13508, 181569),
    ("trex slow", 1, 2): (5753, 39, 65536, 0, 0), ("trex slow", 1, 15): (5753, 39, 62901, 2635, 19968),
    ("trex slow", 1, 32): (5753, 39, 62901, 2635, 39936), ("trex slow", 8, 2): (5753, 31, 62790, 2746, 5208),
    ("trex slow", 8, 15): (5753, 31, 62790, 2746, 21617), ("trex slow", 8, 32): (5753, 31, 62790, 2746, 49277),
    ("trex slow", 12, 2): (5753, 30, 62790, 2746, 5208), ("trex slow", 12, 15): (5753, 30, 62790, 2746, 21531),
    ("trex slow", 12, 32): (5753, 30, 62790, 2746, 49191),
    ("soup z", 1, 2): (65037, 0, 65536, 0, 0), ("soup z", 1, 15): (65037, 0, 7477, 58059, 344334),
    ("soup z", 1, 32): (65037, 0, 6466, 59070, 728536), ("soup z", 8, 2): (65037, 0, 5347, 60189, 118197),
    ("soup z", 8, 15): (65037, 0, 2627, 62909, 655888), ("soup z", 8, 32): (65037, 0, 2247, 63289, 1364457),
    ("soup z", 12, 2): (65037, 0, 7252, 58284, 114275), ("soup z", 12, 15): (65037, 0, 2250, 63286, 635231),
    ("soup z", 12, 32): (65037, 0, 2520, 63016, 1331459),
    ("soup y", 1, 2): (63733, 0, 65536, 0, 0), ("soup y", 1, 15): (63733, 0, 3517, 62019, 481973),
    ("soup y", 1, 32): (63733, 0, 3517, 62019, 969829), ("soup y", 8, 2): (63733, 0, 5475, 60061, 111974),
    ("soup y", 8, 15): (63733, 0, 466, 65070, 771575), ("soup y", 8, 32): (63733, 0, 465, 65071, 1591178),
    ("soup y", 12, 2): (63733, 0, 8823, 56713, 101098), ("soup y", 12, 15): (63733, 0, 1026, 64510, 656551),
    ("soup y", 12, 32): (63733, 0, 287, 65249, 1376926),
}
LARGEST = {"trex fast": 8.7532377243042, "trex slow": 1.7501378059387207, "soup z": 8.14869213104248, "soup y": 21.678}


@pytest.mark.parametrize("taps", [2, 15, 32])
@pytest.mark.parametrize("R", [1, 8, 12])
@pytest.mark.parametrize("pose", list(POSES))
def test_scenes_at_every_radius_and_tap_count(trex256, soup256, filler256, pose, R, taps):
    scene, angles = POSES[pose]
    s = trex256 if scene == "trex" else soup256
    counts = {}
    s.check(filler256, f"{pose}, max_radius {R}, {taps} taps", s.previous(angles), counts=counts, max_radius=R, taps=taps)
    print(f"{pose}, max_radius {R}, {taps} taps: {counts}")
    got = tuple(counts[k] for k in ("moving", "tiles_copied", "copied", "blurred", "taps_taken"))
    assert got == PINNED[pose, R, taps]
    assert counts["largest_l"] == min(float(R), LARGEST[pose]) and counts["copied"] + counts["blurred"] == 256 * 256
    # the conditions, on the pairs at which the model meets them: a twentieth of the frame blurred by the three fast poses
    # whenever an offset can leave the pixel at all, a twentieth copied by the slow one (which blurs 4.2 % of the frame:
    # T-Rex covers 24 % of it and 64 % of that moves by less than a pixel)
    if (R, taps) == (1, 2):
        assert counts["blurred"] == 0
    elif pose == "trex slow":
        assert counts["copied"] >= 0.05 * 256 * 256 and counts["blurred"] >= 0.04 * 256 * 256
    else:
        assert counts["blurred"] >= 0.05 * 256 * 256


def test_the_static_pose_copies_the_frame(trex256, soup256, filler256):
    for s in (trex256, soup256):
        f = filler256
        s.draw(f)
        v = host(f.motion_vectors(s.tri))
        assert_bit_equal(v, s.vectors(s.tri), "the static velocity plane")
        assert 0 < np.abs(v).max() < 1e-4
        for R in (1, 12):
            assert_bit_equal(host(f.motion_blur(s.tri, max_radius=R, taps=32)), s.cam.color_buffer, f"a static pose, max_radius {R}")
        s.check_planes(f, "a static pose")


# ---- 2. hand-built planes through the C entries ----------------------------------------------------------------

class _Planes:
    """Hand-built planes: view depths around 1 in patches, holes, random colours, velocities in patches of their own, and
    random triangles in two poses for the winners to name: what the C entries take.  No rasterizer is involved, so any
    frame shape goes."""

    def __init__(self, oracle, H, W, seed, T=50, holes=0.15, patch=5, speed=20.0):
        rng = np.random.default_rng(seed)
        self.H, self.W, self.T = H, W, T
        self.P = oracle.projection_matrix(45.0, 0.1, 1000.0, max(H, W), max(H, W))    # (any matrix of the shape goes)
        coarse = rng.uniform(0.6, 1.8, ((H + patch - 1) // patch, (W + patch - 1) // patch))
        zv = (np.repeat(np.repeat(coarse, patch, 0), patch, 1)[:H, :W] + rng.uniform(-0.02, 0.02, (H, W))).astype(np.float32)
        self.z = (np.float32(self.P[2, 2]) + np.float32(self.P[3, 2]) / zv).astype(np.float32)
        self.winner = rng.integers(0, T, (H, W)).astype(np.int32)
        self.winner[rng.uniform(size=(H, W)) < holes] = -1
        self.color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
        big = 7
        vc = rng.uniform(-speed, speed, ((H + big - 1) // big, (W + big - 1) // big, 2))
        vc[rng.uniform(size=vc.shape[:2]) < 0.3] = 0
        self.velocity = (np.repeat(np.repeat(vc, big, 0), big, 1)[:H, :W] + rng.uniform(-0.3, 0.3, (H, W, 2))).astype(np.float32)
        self.tri = random_soup(rng, T, 64, size_px=(20.0, 60.0))[0]
        self.prev = (self.tri + rng.uniform(-0.02, 0.02, (T, 1, 3)).astype(np.float32)).astype(np.float32)

    # -- the blur
    def model(self, counts=None, out=None, **kw):
        for k in ("winner", "z", "color", "velocity"):
            kw.setdefault(k, getattr(self, k))
        kw.setdefault("T", self.T)
        start = np.full((self.H, self.W, 3), np.nan, np.float32) if out is None else out
        return motion_ref.motion_blur(kw.pop("color"), kw.pop("winner"), kw.pop("z"), kw.pop("T"), self.P, kw.pop("velocity"),
                                      counts=counts, out=start, **kw)

    def device(self, max_radius=8, taps=16, soft=0.02, T=None, y0=0, y1=None, out=None, **planes):
        """The result plane of crender_motion_blur (rows outside y0 .. y1 are `out`'s, NaN without one)."""
        import torch
        from cython3dmodelrenderer_amd import _capi
        L = _capi.load()
        kept = {k: np.ascontiguousarray(planes.get(k, getattr(self, k))) for k in ("winner", "z", "color", "velocity")}
        dev = {k: torch.from_numpy(v).cuda() for k, v in kept.items()}
        d_out = torch.from_numpy(np.full((self.H, self.W, 3), np.nan, np.float32) if out is None else np.ascontiguousarray(out)).cuda()
        T = self.T if T is None else T
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(L.crender_motion_blur(dev["winner"].data_ptr(), dev["z"].data_ptr(), None, T, None, _capi.f32_16(self.P),
                                          dev["color"].data_ptr(), dev["velocity"].data_ptr(), max_radius, taps, soft,
                                          d_out.data_ptr(), self.H, self.W, y0, self.H if y1 is None else y1, 0, st),
                    "crender_motion_blur")
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

    # -- the vectors
    def vectors_model(self, exposure=1.0, y0=0, y1=None, T=None, winner=None):
        T = self.T if T is None else T
        start = np.full((self.H, self.W, 2), np.nan, np.float32)
        return motion_ref.motion_vectors(self.winner if winner is None else winner, self.tri[:T], self.P, self.prev[:T],
                                         exposure, y0, y1, out=start)

    def vectors_device(self, exposure=1.0, y0=0, y1=None, T=None, winner=None):
        import torch
        from cython3dmodelrenderer_amd import _capi
        L = _capi.load()
        T = self.T if T is None else T
        win = torch.from_numpy(np.ascontiguousarray(self.winner if winner is None else winner)).cuda()
        tri, prev = torch.from_numpy(self.tri).cuda(), torch.from_numpy(self.prev).cuda()
        d_out = torch.from_numpy(np.full((self.H, self.W, 2), np.nan, np.float32)).cuda()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(L.crender_motion_vectors(win.data_ptr(), tri.data_ptr() if T else None, T, None, _capi.f32_16(self.P),
                                             prev.data_ptr() if T else None, exposure, d_out.data_ptr(), self.H, self.W, y0,
                                             self.H if y1 is None else y1, 0, st), "crender_motion_vectors")
        return host(d_out)

    def check_vectors(self, what, **kw):
        want = self.vectors_model(**kw)
        assert np.isfinite(want[~np.isnan(want)]).all() and (want[~np.isnan(want)] != 0).any(), what
        assert_bit_equal(self.vectors_device(**kw), want, what)


# 5 x 7, 1 x 40 and 40 x 1: frames smaller than the halo.  33 x 65: one pixel taller and one pixel wider than whole tiles
# of 32.  63 x 31: a partial tile in both directions.
@pytest.mark.parametrize("H,W", [(5, 7), (1, 40), (40, 1), (33, 65), (63, 31)])
def test_frames_that_do_not_fit_the_tiles(oracle, H, W):
    p = _Planes(oracle, H, W, seed=80 + H)
    if H == 1 or W == 1:
        p.velocity[..., 1 if H == 1 else 0] *= np.float32(0.05)        # along the line, or every offset leaves the frame
    p.check_vectors(f"{H} x {W}: the vectors")
    p.check_vectors(f"{H} x {W}: the vectors at half the exposure", exposure=0.5)
    for R in (1, 12):
        for taps in (2, 15, 32):
            p.check(f"{H} x {W}, max_radius {R}, {taps} taps", max_radius=R, taps=taps, min_blurred=0 if R == 1 or taps == 2 else 1)
        if H > 8:
            p.check(f"{H} x {W}, max_radius {R}, rows 3 .. {H - 2}", max_radius=R, taps=9, y0=3, y1=H - 2)
            p.check_vectors(f"{H} x {W}: the vectors of rows 3 .. {H - 2}", y0=3, y1=H - 2)


def test_a_frame_of_more_tiles_than_the_blur_grid_holds(oracle):
    """A launch is at most 2048 workgroups, each looping over tiles of 32 x 32: a frame 3 pixels wide and 65 600 tall is
    2050 tiles, so two workgroups make a second trip."""
    p = _Planes(oracle, 65600, 3, seed=91)
    counts = p.check("65600 x 3", max_radius=2, taps=5, min_blurred=1000)
    assert counts["copied"] > 1000
    want = p.model(max_radius=2, taps=5)
    assert (want[65536:].view(np.uint32) != p.color[65536:].view(np.uint32)).any()          # the second trip's rows


def test_a_frame_of_more_row_blocks_than_the_vector_grid_holds(oracle):
    """The vector kernel's grid is at most 65 535 row blocks of 8 rows tall and loops over the rest: a frame 1 pixel wide and
    524 300 tall is 65 538 row blocks, so three of them are a second trip (and the blur's grid makes eight trips)."""
    p = _Planes(oracle, 524300, 1, seed=92)
    want = p.vectors_model()
    assert (want[65535 * 8:] != 0).any()
    assert_bit_equal(p.vectors_device(), want, "524300 x 1: the vectors")
    p.check("524300 x 1: the blur", max_radius=3, taps=4, min_blurred=1000)


# ---- 3. hand-built velocity planes -----------------------------------------------------------------------------

def _still(oracle, H=96, W=96, seed=5):
    p = _Planes(oracle, H, W, seed=seed, holes=0.1)
    p.velocity = np.zeros((H, W, 2), np.float32)
    return p


def test_the_dominant_direction_in_every_octant_and_along_both_axes(oracle):
    p = _still(oracle)
    for k, (vx, vy) in enumerate([(14, 0), (-14, 0), (0, 14), (0, -14), (12, 5), (5, 12), (-5, 12), (-12, 5), (-12, -5), (-5, -12),
                                  (5, -12), (12, -5), (10, 10), (-10, 10)]):
        v = p.velocity.copy()
        v[:, :, 0], v[:, :, 1] = vx, vy
        v[::3, ::2] *= np.float32(0.25)                 # slower pixels among them: other il, the same taps
        for R, taps in ((8, 16), (12, 31), (3, 32)):
            c = p.check(f"direction {(vx, vy)}, max_radius {R}, {taps} taps", velocity=v, max_radius=R, taps=taps, min_blurred=5000)
            assert c["tiles_copied"] == 0


def test_products_on_a_half_take_rints_tie(oracle):
    """D = (8, 0) with 16 taps puts D * tau on 7.5, 6.5, ..., which go to the even neighbour; D = (3, -5) with 2 taps on
    (-1.5, 2.5) and (1.5, -2.5): (-2, 2) and (2, -2)."""
    p = _still(oracle)
    # ((2, 2) at max_radius 1 clamps to D = (0.71, 0.71): the offsets (+-1, +-1) lie at dist 1.41 > l = 1, where cone and
    # cylinder are 0: taps that are walked and never taken.  (5, 0) with 2 taps: 2.5 * -+0.5 = -+1.25, not a tie.)
    for (vx, vy), R, taps, least in (((16, 0), 8, 16, 1000), ((0, -16), 8, 16, 1000), ((6, -10), 12, 2, 1000), ((24, 24), 12, 8, 1000),
                                     ((2, 2), 1, 4, 0), ((5, 0), 4, 2, 1000), ((3, 0), 4, 6, 1000)):
        v = p.velocity.copy()
        v[:] = np.float32([vx, vy])
        p.check(f"ties, v {(vx, vy)}, max_radius {R}, {taps} taps", velocity=v, max_radius=R, taps=taps, min_blurred=least)
    ox, oy, _ = motion_ref.tile_taps(np.float32(8), np.float32(0), 16, 8)
    assert ox.tolist() == [-8, -6, -6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6, 6, 8]


def test_which_pixel_is_dominant(oracle):
    p = _still(oracle)
    # two staged pixels of equal largest l: the first in frame order wins, whatever wavefront staged it
    for first, second in (((40, 50), (40, 45)), ((39, 60), (40, 33)), ((33, 33), (62, 62)), ((30, 70), (31, 20)), ((50, 31), (50, 32))):
        v = p.velocity.copy()
        v[first[0], first[1]], v[second[0], second[1]] = (0, 10), (10, 0)
        v[45:55, 45:55] = (3, 3)                        # something slower that is blurred along whichever wins
        dom = []
        p.model(velocity=v, max_radius=8, dominant=dom)
        lo = min(first, second)
        assert (32, 32, lo[1], lo[0]) in dom
        p.check(f"equal l at {first} and {second}", velocity=v, max_radius=8, taps=16, min_blurred=50)
    # the dominant pixel in the halo and in the halo's corner of the centre tile, at the smallest and the largest halo
    for at in ((31, 40), (40, 31), (31, 31), (64, 64), (31, 64), (20, 20), (75, 75), (20, 75)):
        v = p.velocity.copy()
        v[at] = (9, -1)                                 # (near an axis, and the block at l >= 1: at max_radius 1 only offsets
        v[40:56, 40:56] = (2.5, 0.5)                    # of dist 1 between pixels clamped to l = 1 weigh at all)
        for R in (1, 8, 12):
            p.check(f"the dominant pixel at {at}, max_radius {R}", velocity=v, max_radius=R, taps=15, min_blurred=1)
    # a lone fast pixel on a tile seam, another one with another direction on the next seam: neighbouring tiles gather
    # along different directions
    v = p.velocity.copy()
    v[:] = (6, 2)
    v[31, 31], v[64, 70], v[10, 64] = (20, 0), (0, 20), (-14, 14)
    dom = []
    c = {}
    p.model(velocity=v, max_radius=8, taps=16, dominant=dom, counts=c)
    assert len({d[2:] for d in dom}) >= 3 and c["blurred"] > 5000
    p.check("lone fast pixels on the seams", velocity=v, max_radius=8, taps=16)


def test_the_threshold_of_a_half_and_odd_velocities(oracle):
    p = _still(oracle)
    one = np.float32(1.0)
    v = p.velocity.copy()
    v[..., 0] = one                                     # l is exactly 1/2 everywhere: every tile copies
    assert_bit_equal(p.device(velocity=v, max_radius=4, taps=32), p.color, "l = 1/2 copies")
    v[40, 40, 0] = np.nextafter(one, np.float32(2))     # the next float above, seen by one tile: that tile walks its taps,
    c = p.check("the next float above 1/2", velocity=v, max_radius=4, taps=32, min_blurred=0)      # whose offsets are all (0, 0)
    assert c["tiles_copied"] == 8 and c["moving"] == 1 and c["blurred"] == 0
    v[41, 41] = (3, 0)                                  # and with a faster pixel beside it the tile blurs
    c = p.check("a faster pixel beside it", velocity=v, max_radius=4, taps=32)
    assert c["tiles_copied"] == 8 and c["moving"] == 2
    # l above max_radius, 1e30, +-inf and NaN
    rng = np.random.default_rng(3)
    v = p.velocity.copy()
    v[:] = rng.uniform(-40, 40, v.shape).astype(np.float32)
    hit = rng.uniform(size=v.shape[:2]) < 0.1
    v[hit] = rng.choice(np.float32([1e30, -1e30, np.inf, -np.inf, np.nan, 3e38, 1e19]), (int(hit.sum()), 2))
    for R, taps in ((1, 7), (8, 16), (12, 32)):
        c = p.check(f"odd velocities, max_radius {R}", velocity=v, max_radius=R, taps=taps, min_blurred=1000)
        assert c["largest_l"] == R
    v[:] = np.float32([1e30, -1e30])                    # every D is (0, 0): the clamp's R / inf
    assert_bit_equal(p.device(velocity=v, max_radius=8, taps=16), p.color, "1e30 everywhere copies")


# ---- 4. special values -----------------------------------------------------------------------------------------

def _assert_equal_up_to_computed_nans(got, want, blurred, what):
    """Bit for bit, but where the model COMPUTED a NaN (a blurred pixel that took a NaN or an infinite colour): there the
    kernel has a NaN as well, whose sign and payload the contract leaves open (the host's and the device's differ).  A
    copied pixel keeps every bit of its NaNs."""
    computed = np.isnan(want) & blurred[..., None]
    assert np.isnan(got[computed]).all(), what
    assert_bit_equal(np.where(computed, np.float32(0), got), np.where(computed, np.float32(0), want), what)


def test_special_values_through_the_c_entries(oracle):
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
    for kw in (dict(max_radius=1, taps=5), dict(max_radius=8, taps=16), dict(max_radius=12, taps=32), dict(max_radius=8, taps=16, soft=1e-30),
               dict(max_radius=8, taps=16, soft=1e30), dict(max_radius=4, taps=3, soft=1.0)):
        blurred = np.zeros((H, W), bool)
        want = p.model(mask=blurred, **odd, **kw)
        seen["computed"] |= bool(np.isnan(want[blurred]).any())
        seen["copied"] |= bool(np.isnan(want[~blurred]).any())
        assert np.isinf(want).any() and blurred.sum() > 50
        _assert_equal_up_to_computed_nans(p.device(**odd, **kw), want, blurred, f"odd values, {kw}")
    assert seen == dict(computed=True, copied=True)                  # NaNs that were taken, and NaNs that were copied
    # a zero velocity plane: the copy keeps -0, the infinities and every NaN
    assert_bit_equal(p.device(velocity=np.zeros((H, W, 2), np.float32), max_radius=12, **odd), color, "no velocity over odd values")
    # T = 0 and a frame that is background only: every depth is the stand-in, the velocities still blur
    for what, planes in (("T == 0", dict(T=0)), ("background only", dict(winner=np.full((H, W), -1, np.int32)))):
        counts = {}
        want = p.model(counts=counts, max_radius=8, z=z, **planes)
        assert counts["covered"] == 0 and counts["blurred"] > 500
        assert_bit_equal(p.device(max_radius=8, z=z, **planes), want, what)
    # the vectors: invalid winners, T == 0, background only and exposure 0 give zeros where they must
    want = p.vectors_model(winner=winner)
    invalid = (winner < 0) | (winner >= T)
    assert not want[invalid].any() and not np.signbit(want[invalid]).any() and want[~invalid].any()
    assert_bit_equal(p.vectors_device(winner=winner), want, "the vectors under invalid winners")
    for what, kw in (("T == 0", dict(T=0)), ("background only", dict(winner=np.full((H, W), -1, np.int32)))):
        got = p.vectors_device(**kw)
        assert not got.any() and not np.signbit(got).any(), what
    assert_bit_equal(p.vectors_device(exposure=0.0), p.vectors_model(exposure=0.0), "exposure 0")
    assert not p.vectors_device(exposure=0.0).any()
    # a previous pose behind the camera, at z = 0 and with NaN corners: no velocity
    keep = p.prev
    try:
        p.prev = keep.copy()
        p.prev[::3, :, 2] = -1.0
        p.prev[1::3, :, 2] = 0.0
        p.prev[2::3, 0, 0] = np.nan
        want = p.vectors_model()
        assert_bit_equal(p.vectors_device(), want, "odd previous poses")
    finally:
        p.prev = keep


# ---- 5. a row strip --------------------------------------------------------------------------------------------

def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_zero(oracle):
    import torch
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    prev = s.previous((0, 10, 0))
    f = filler(200, 173, row_strip=(y0, y1))
    s.draw(f)
    f.synchronize()
    v = f.motion_vectors(prev)
    want_v = s.vectors(prev, y0=y0, y1=y1)
    assert not host(v)[:y0].any() and not host(v)[y1:].any()
    assert_bit_equal(host(v), want_v, "the strip's vectors")
    # rows outside the strip: colours, winners, depths and velocities that WOULD show if the pass read them
    f.color_buffer[:y0] = 7.5e3
    f.color_buffer[y1:] = -2.25e3
    f.winner_buffer[:y0] = 0
    f.winner_buffer[y1:] = 1
    f.z_buffer[:y0] = float(s.cam.z_buffer[s.cam.winner >= 0].min())
    f.z_buffer[y1:] = float("nan")
    poisoned = v.clone()
    poisoned[:y0] = torch.tensor([0.0, 30.0], device=v.device)
    poisoned[y1:] = torch.tensor([-30.0, -30.0], device=v.device)
    kw = dict(max_radius=8, taps=16)
    got = host(f.motion_blur(velocity=poisoned, **kw))
    assert not got[:y0].any() and not got[y1:].any()
    counts = {}
    want = s.want(want_v, y0=y0, y1=y1, counts=counts, **kw)
    assert counts["blurred"] > 1000 and counts["copied"] > 1000
    assert_bit_equal(got[y0:y1], want[y0:y1], "the strip's rows")
    # the poison works: a pass that looked across the strip's edge would give other colours
    seen = motion_ref.motion_blur(host(f.get_color_tensor()), host(f.get_winner_tensor()), host(f.get_z_tensor()), len(s.tri),
                                  s.cam.proj_mat, host(poisoned), **kw)
    assert (seen[y0:y1].view(np.uint32) != want[y0:y1].view(np.uint32)).any()
    assert_bit_equal(host(f.get_color_tensor())[y0:y1], s.cam.color_buffer[y0:y1], "the colour plane is only read")
    # and the vectors do not read the winners outside either
    again = host(f.motion_vectors(prev))
    assert_bit_equal(again, want_v, "the strip's vectors over poisoned rows")


# ---- 6. the filler ---------------------------------------------------------------------------------------------

KW = dict(max_radius=6, taps=12, soft=0.05)
ANGLES = (0, 0, 5)


def test_host_view_edits_reach_the_pass(soup256, filler256):
    s, f = soup256, filler256
    prev = s.previous(ANGLES)
    v = s.vectors(prev)
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    out = f.motion_blur(prev, **KW)
    want = s.want(v, **KW)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(out), want, "the plain pass")
    assert f.get_color_buffer() is view
    assert_bit_equal(view, s.cam.color_buffer, "the view still shows the frame")
    # velocity= of motion_vectors' own result equals previous_vertices=, and an edited plane is what is walked
    mine = f.motion_vectors(prev)
    assert_bit_equal(host(f.motion_blur(velocity=mine, **KW)), want, "velocity= of motion_vectors' result")
    doubled = s.want(v * np.float32(2), **KW)
    assert (doubled != want).any()
    assert_bit_equal(host(f.motion_blur(velocity=mine * 2, **KW)), doubled, "an edited velocity plane")
    assert_bit_equal(host(f.motion_blur(velocity=v * np.float32(2), **KW)), doubled, "a numpy velocity plane")
    assert_bit_equal(host(f.motion_blur(prev, exposure=2.0, **KW)), s.want(s.vectors(prev, exposure=2.0), **KW), "exposure 2")
    # an edit of the colour view reaches the pass (the view asked for again: the passes above have carried up what was
    # exposed before them, and an edit counts from a getter's call on)
    assert f.get_color_buffer() is view
    view[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    edited = s.cam.color_buffer.copy()
    edited[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    want_c = s.want(v, color=edited, **KW)
    assert (want_c != want).any()
    assert_bit_equal(host(f.motion_blur(prev, **KW)), want_c, "over edited colours")
    # and one of the z view: a block pushed far behind no longer spreads over its surroundings
    s.draw(f)
    zb = f.get_z_buffer()
    block = s.cam.z_buffer.copy()
    block[100:140, 100:140] = np.float32(s.cam.proj_mat[2, 2]) + np.float32(s.cam.proj_mat[3, 2]) / np.float32(30.0)
    zb[:] = block
    want_z = motion_ref.motion_blur(s.cam.color_buffer, s.cam.winner, block, len(s.tri), s.cam.proj_mat, v, **KW)
    assert (want_z != want).any()
    assert_bit_equal(host(f.motion_blur(prev, **KW)), want_z, "under an edited z")
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
    prev = s.previous((0, 8, 0))
    v = s.vectors(prev)
    kw = dict(max_radius=8, taps=16)
    want = s.want(v, **kw)
    assert (want != s.cam.color_buffer).any()
    f = filler(256, 256)                          # numpy
    s.draw(f)
    assert_bit_equal(host(f.motion_vectors(prev)), v, "numpy inputs: the vectors")
    assert_bit_equal(host(f.motion_blur(prev, **kw)), want, "numpy inputs")
    s.check_planes(f, "numpy inputs")
    f = filler(256, 256)                          # caller's device tensors
    f.render_arrays(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (tri, col, nrm)], clear=True)
    d_prev = torch.from_numpy(prev).cuda()
    assert_bit_equal(host(f.motion_vectors(d_prev)), v, "torch inputs: the vectors")
    assert_bit_equal(host(f.motion_blur(d_prev, **kw)), want, "torch inputs")
    f = filler(256, 256)                          # the device-resident model
    f.render_model(DeviceModel(m), clear=True)
    assert_bit_equal(host(f.motion_blur(d_prev, **kw)), want, "DeviceModel inputs")
    s.check_planes(f, "DeviceModel inputs")


def test_a_frame_redrawn_after_a_bin_overflow_ends_blurred(oracle):
    """The scene of test_a_frame_redrawn_after_a_bin_overflow_ends_lit: the bin lists are far too small, the frame drops
    fragments and is rendered again when it is settled — which the pass does before it launches.  With presort the
    frame's triangles are reordered and the vectors go through d_pos_of."""
    s = _Scene(oracle, random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0), 512, 512)
    prev = s.previous((0, 0, 2))
    kw = dict(max_radius=8, taps=8)
    v = s.vectors(prev)
    want = s.want(v, **kw)
    assert (want != s.cam.color_buffer).any()
    for more in (dict(), dict(presort=True)):
        f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False, **more)
        s.draw(f)
        need, cap = f.bin_usage()
        assert cap == 500 and need > cap and len(f._pending) == 1     # dropped fragments, nobody has looked yet
        out = f.motion_blur(prev, **kw)
        assert not f._pending                                          # grown and redone before the pass
        assert_bit_equal(host(out), want, f"a redone frame, {more}")
        assert_bit_equal(host(f.motion_vectors(prev)), v, f"a redone frame's vectors, {more}")
        s.check_planes(f, "a redone frame")


# ---- 7. Renderer -----------------------------------------------------------------------------------------------

MB = dict(max_radius=6, taps=12, soft=0.05)


class _Turning:
    """The soup as a model whose vertex array is replaced by a rotated one between two frames."""

    def __init__(self, s):
        self._vertices_by_triangles, self._colors_by_triangles, self._normals_by_triangles = s.previous(ANGLES), s.col, s.nrm
        self._after = s.tri

    def turn(self):
        self._vertices_by_triangles = self._after


def _two_frames(r, s):
    """Two render calls of the soup, rotated in between: (the first image, the second)."""
    m = _Turning(s)
    first = r.render(m)
    first = np.array(first) if isinstance(first, np.ndarray) else host(first)
    m.turn()
    second = r.render(m)
    return first, (np.array(second) if isinstance(second, np.ndarray) else host(second)), m


@pytest.mark.parametrize("on_device", [None, True, "fused"])
def test_renderer_with_guro_illumination(oracle, soup256, on_device):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    prev = s.previous(ANGLES)
    lit = oracle.guro(s.cam.color_buffer.copy(), s.cam.normals_buffer, GURO)
    want = s.want(s.vectors(prev), color=lit, **MB)
    assert (want != lit).any()
    f = filler(256, 256)
    r = Renderer(f, GuroIllumination(GURO), on_device=on_device, motion_blur=MB)
    first, second, m = _two_frames(r, s)
    assert isinstance(r.render(m), np.ndarray) == (on_device is None)
    assert np.array_equal(second, want, equal_nan=True)          # as values: the light leaves -0 on the background
    s.check_planes(f, "after Renderer")
    # the first call copies its frame: the previous pose drawn and lit, unblurred
    b = filler(256, 256)
    b.set_fused_illumination(GuroIllumination(GURO).light_direction)
    b.render_arrays(prev, s.col, s.nrm, clear=True)
    assert np.array_equal(first, host(b.get_color_tensor()), equal_nan=True)
    # a third call of the same pose is static, and so is the call after reset_motion()
    third = r.render(m)
    third = np.array(third) if on_device is None else host(third)
    assert np.array_equal(third, lit, equal_nan=True)
    m._vertices_by_triangles = prev
    r.reset_motion()
    again = r.render(m)
    assert np.array_equal(np.array(again) if on_device is None else host(again), first, equal_nan=True)
    if on_device == "fused":                       # and by hand, bit for bit: the raster kernel shades, then the pass
        a = filler(256, 256)
        a.set_fused_illumination(GuroIllumination(GURO).light_direction)
        s.draw(a)
        assert_bit_equal(second, host(a.motion_blur(prev, **MB)), "the fused light, then motion_blur")


PHONG_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.25)]
PHONG_KW = dict(ambient=0.15, shininess=16)


def test_renderer_after_the_phong_pass_and_with_bloom_after_it(soup256):
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    prev = s.previous(ANGLES)
    lit = phong_ref.phong_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.cam.normals_buffer, PHONG_LIGHTS, **PHONG_KW)
    want = s.want(s.vectors(prev), color=lit, **MB)
    assert (want != lit).any()
    f = filler(256, 256)
    r = Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, **PHONG_KW), on_device=True, motion_blur=MB)
    _, second, _ = _two_frames(r, s)
    assert_bit_equal(second, want, "Renderer(PhongIllumination, motion_blur=...)")
    # with bloom after it: the passes by hand
    glow = dict(threshold=150.0, radius=4)
    f = filler(256, 256)
    r = Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, **PHONG_KW), on_device=True, motion_blur=MB, bloom=glow)
    _, second, _ = _two_frames(r, s)
    a = filler(256, 256)
    s.draw(a)
    a.phong_pass(PHONG_LIGHTS, **PHONG_KW)
    blurred = a.motion_blur(prev, **MB)
    assert_bit_equal(host(blurred), want, "phong_pass, then motion_blur")
    by_hand = host(a.bloom(source=blurred, **glow))
    assert (by_hand != want).any()
    assert_bit_equal(second, by_hand, "phong_pass, motion_blur, then bloom")
    s.check_planes(a, "after the passes")


# ---- 8. errors -------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(soup256):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    prev = s.previous(ANGLES)
    f = filler(256, 256, track_winner=False)
    s.draw(f)
    with pytest.raises(ValueError, match="motion_blur needs the winner plane"):
        f.motion_blur(prev)
    with pytest.raises(ValueError, match="motion_vectors needs the winner plane"):
        f.motion_vectors(prev)
    f = filler(256, 256)
    with pytest.raises(ValueError, match="motion_blur: no frame has been rendered"):
        f.motion_blur(prev)
    s.draw(f)
    f.render_arrays(s.tri, s.col, s.nrm)           # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.motion_vectors(prev)
    with pytest.raises(ValueError, match="motion_blur is not available on a swap chain"):
        filler(64, 64, pipeline=True).motion_blur(prev)
    s.draw(f)
    T = len(s.tri)
    with pytest.raises(ValueError, match=f"previous_vertices holds {T - 2} triangles, the last frame drew {T}"):
        f.motion_blur(prev[2:])
    with pytest.raises(ValueError, match="exactly one of previous_vertices and velocity"):
        f.motion_blur()
    with pytest.raises(ValueError, match="exactly one of previous_vertices and velocity"):
        f.motion_blur(prev, velocity=np.zeros((256, 256, 2), np.float32))
    with pytest.raises(ValueError, match="velocity must be float32"):
        f.motion_blur(velocity=np.zeros((256, 255, 2), np.float32))
    with pytest.raises(ValueError, match="exposure=2.0 with velocity="):
        f.motion_blur(velocity=np.zeros((256, 256, 2), np.float32), exposure=2.0)
    for bad in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="exposure must be a finite number, 0 or above"):
            f.motion_vectors(prev, exposure=bad)
    for bad in (0, 13, 8.0, True):
        with pytest.raises(ValueError, match="max_radius must be an int from 1 to 12"):
            f.motion_blur(prev, max_radius=bad)
    for bad in (0, 33, 16.0, True):
        with pytest.raises(ValueError, match="taps must be an int from 1 to 32"):
            f.motion_blur(prev, taps=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="soft must be a finite range of view depths above 0"):
            f.motion_blur(prev, soft=bad)
    guro = GuroIllumination(GURO)
    for other in (dict(antialias={}), dict(depth_of_field=dict(focus=1.0)), dict(supersample=2), dict(transparency=dict(alpha=0.5))):
        with pytest.raises(ValueError, match="motion_blur.*together with antialias"):
            Renderer(f, guro, motion_blur=MB, **other)
    with pytest.raises(ValueError, match=r"\['shutter'\] unknown"):
        Renderer(f, guro, motion_blur=dict(MB, shutter=1))
    with pytest.raises(ValueError, match="object has no motion_blur"):
        Renderer(object(), guro, motion_blur=MB)
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "nothing was written")
    out = f.motion_blur(prev, **MB)                # and works again
    want = s.want(s.vectors(prev), **MB)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(out), want, "after the errors")
    s.check_planes(f, "after the errors")
