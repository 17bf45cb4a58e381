"""The ambient-occlusion pass on the GPU (csrc/ao.hip through AdvancedPixelBufferFiller.ao_pass and Renderer), bit for
bit against the host model of tests/ao_ref.py evaluated on the oracle's frames (itself pinned in tests/test_ao_cpu.py).
Every test asserts that z, normals and winners are unchanged and that the pass changed something."""
import ctypes as C
import os

import numpy as np
import pytest

import ao_ref
import phong_ref
import shadow_ref
from pass_scenes import GOLDEN, Scene, filler, host, soup_fixture, trex_arrays, trex_fixture
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)
TABLE = [(1, 0), (-2, 2), (0, -3), (2, 3), (-4, -1), (4, -3), (-1, 5), (-3, -5), (5, 2), (-6, 2), (3, -6), (2, 6), (-6, -4),
         (7, -2), (-4, 6), (-1, -8)]
SOUP_KW = dict(radius=0.05, radius_px=8, strength=3.0, floor=0.25)


def _table(kw):
    """The tap table of ao_pass's arguments, as the filler builds it."""
    from cython3dmodelrenderer_amd import ambient_occlusion
    taps = kw.get("taps", 16)
    return ambient_occlusion.taps(kw.get("radius_px", 8), taps) if isinstance(taps, int) else list(taps)


def _model_kw(kw):
    """ao_pass's arguments (and its defaults) as ao_ref.ao_pass takes them."""
    m = dict(radius=0.03, radius_px=8, min_cos=0.1, strength=2.0, floor=0.0, rotate=True)
    m.update({k: v for k, v in kw.items() if k not in ("taps", "normals")})
    m["face"] = kw.get("normals", "plane") == "face"
    return m


class _Scene(Scene):
    def want(self, color=None, counts=None, y0=0, y1=None, **kw):
        out = ao_ref.ao_pass(self.cam.color_buffer if color is None else color, self.cam.z_buffer, self.cam.winner,
                             self.tri, self.cam.proj_mat, self.cam.normals_buffer, _table(kw), y0=y0, y1=y1, counts=counts,
                             **_model_kw(kw))
        assert not np.isnan(out).any()
        return out

    def check(self, f, what, counts=None, **kw):
        self.draw(f)
        f.ao_pass(**kw)
        want = self.want(counts=counts, **kw)
        self.assert_changed(want, what)
        assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour")
        self.check_planes(f, what)
        return want


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


@pytest.fixture(scope="module")
def filler256():
    return filler(256, 256)


# ---- 1. T-Rex ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("normals", ["plane", "face"])
def test_trex_every_instance(trex256, filler256, normals, rotate):
    s = trex256
    assert s.covered == 15801
    counts = {}
    s.check(filler256, f"trex256, {normals}, rotate={rotate}", counts=counts, taps=TABLE, radius=0.03, strength=1.0,
            normals=normals, rotate=rotate)
    if normals == "plane":
        assert (counts["occluded"], counts["taps_taken"]) == ((7102, 22461) if rotate else (7245, 22514))


# (1, 1) .. (64, 32): every tap count at every halo it fits in; the world radius grows with the halo so that the far
# taps are taken
@pytest.mark.parametrize("taps,radius_px", [(1, 1), (8, 1), (1, 8), (16, 8), (64, 8), (1, 32), (16, 32), (64, 32)])
def test_trex_tap_counts_and_radii(trex256, filler256, taps, radius_px):
    counts = {}
    kw = dict(taps=taps, radius_px=radius_px, radius={1: 0.01, 8: 0.03, 32: 0.12}[radius_px], strength=1.5)
    trex256.check(filler256, f"trex256, {taps} taps in {radius_px} px", counts=counts, **kw)
    trex256.check(filler256, f"trex256, {taps} taps in {radius_px} px, face, unrotated", normals="face", rotate=False, **kw)
    assert counts["taps_taken"] > 0


@pytest.mark.parametrize("R", [1, 8, 32])
def test_trex_the_corners_and_the_edges_of_the_halo(trex256, filler256, R):
    table = [(R, R), (-R, R), (R, -R), (-R, -R), (R, 0), (-R, 0), (0, R), (0, -R)]
    for rotate in (True, False):
        for one in (table, table[:4], table[4:]):
            counts = {}
            trex256.check(filler256, f"halo {R}, rotate={rotate}, {one}", counts=counts, taps=one, radius_px=R,
                          radius=0.006 * R, rotate=rotate, strength=1.0)
            assert counts["taps_taken"] > 100


# ---- 2. shapes where staging can go wrong ----------------------------------------------------------------------

def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_alone(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    near = float(s.cam.z_buffer[s.cam.winner >= 0].min()) - 1e-3
    for normals in ("plane", "face"):
        s.draw(f)
        f.synchronize()
        # rows outside the strip: colours to be kept, and winners and depths that WOULD occlude if the pass read them
        f.color_buffer[:y0] = 7.5
        f.color_buffer[y1:] = -2.25
        f.winner_buffer[:y0] = 0
        f.winner_buffer[y1:] = 1
        f.z_buffer[:y0] = near
        f.z_buffer[y1:] = near
        kw = dict(taps=TABLE, radius=0.2, strength=1.0, normals=normals)
        f.ao_pass(**kw)
        got = host(f.get_color_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        want = s.want(y0=y0, y1=y1, **kw)
        assert (want[y0:y1].view(np.uint32) != s.cam.color_buffer[y0:y1].view(np.uint32)).any()
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, {normals}")
        # the poison works: a pass that looked across the strip's edge would give other colours
        poisoned_w, poisoned_z = host(f.get_winner_tensor()), host(f.get_z_tensor())
        seen = ao_ref.ao_pass(s.cam.color_buffer, poisoned_z, poisoned_w, s.tri, s.cam.proj_mat, s.cam.normals_buffer, TABLE,
                              **_model_kw(kw))
        assert (seen[y0:y1] != want[y0:y1]).any()
        assert_bit_equal(poisoned_w[y0:y1], s.cam.winner[y0:y1], "winner")
        assert_bit_equal(poisoned_z[y0:y1], s.cam.z_buffer[y0:y1], "z")
        assert_bit_equal(host(f.get_normals_tensor()), s.cam.normals_buffer, "normals")


class _Planes:
    """Hand-built planes of a bumpy surface with holes, and a triangle per pixel class for the face mode: what the C
    entry takes.  No rasterizer is involved, so any frame shape goes."""

    def __init__(self, oracle, H, W, seed, T=50, holes=0.15):
        rng = np.random.default_rng(seed)
        self.H, self.W, self.T = H, W, T
        self.P = oracle.projection_matrix(45.0, 0.1, 1000.0, max(H, W), max(H, W))    # (any matrix of the shape goes)
        # view depths around 1 with a relief of a few pixel widths
        c = ao_ref.constants(self.P, W, H, 1.0, 1)
        px = float(min(abs(c[2]), abs(c[3])))          # (pixels are oblong where the frame is)
        zv = (1.0 + px * rng.uniform(-3, 3, (H, W))).astype(np.float32)
        self.z = (np.float32(self.P[2, 2]) + np.float32(self.P[3, 2]) / zv).astype(np.float32)
        self.winner = rng.integers(0, T, (H, W)).astype(np.int32)
        self.winner[rng.uniform(size=(H, W)) < holes] = -1
        self.normal = rng.standard_normal((H, W, 3)).astype(np.float32)
        self.normal[..., 2] = -np.abs(self.normal[..., 2]) - 0.5
        self.tri = rng.uniform(-1, 1, (T, 3, 3)).astype(np.float32)
        self.tri[..., 2] += 2.0
        self.color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
        self.radius = 6 * px

    def model(self, table, counts=None, **kw):
        kw.setdefault("radius", self.radius)
        for k in ("winner", "z", "normal", "tri", "color"):
            kw.setdefault(k, getattr(self, k))
        return ao_ref.ao_pass(kw.pop("color"), kw.pop("z"), kw.pop("winner"), kw.pop("tri"), self.P, kw.pop("normal"), table,
                              counts=counts, **kw)

    def device(self, table, face=False, rotate=True, radius=None, radius_px=8, min_cos=0.1, strength=2.0, floor=0.0, T=None,
               pos_of=None, y0=0, y1=None, **planes):
        """The colours after crender_ao_shade, and the other planes as the device holds them afterwards."""
        import torch
        from cython3dmodelrenderer_amd import _capi
        lib = _capi.load()
        kept = {k: np.ascontiguousarray(planes.get(k, getattr(self, k))) for k in ("winner", "z", "normal", "tri", "color")}
        dev = {k: torch.from_numpy(v).cuda() for k, v in kept.items()}
        T = self.T if T is None else T
        d_pos = None if pos_of is None else torch.from_numpy(np.ascontiguousarray(pos_of).view(np.int32)).cuda()
        taps2 = (C.c_int8 * (2 * len(table)))(*[v for p in table for v in p])
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        flags = (_capi.AO_ROTATE if rotate else 0) | (_capi.AO_FACE_NORMALS if face else 0)
        _capi.check(lib.crender_ao_shade(
            dev["winner"].data_ptr(), dev["z"].data_ptr(), dev["tri"].data_ptr() if T else None, T,
            None if d_pos is None else d_pos.data_ptr(), _capi.f32_16(self.P), dev["normal"].data_ptr(), taps2, len(table),
            radius_px, self.radius if radius is None else radius, min_cos, strength, floor, dev["color"].data_ptr(),
            self.H, self.W, y0, self.H if y1 is None else y1, flags, st), "crender_ao_shade")
        got = host(dev["color"])
        for k in ("winner", "z", "normal", "tri"):
            assert_bit_equal(host(dev[k]), kept[k], f"{k} is only read")
        return got

    def check(self, what, table=TABLE + [(0, 1), (-1, 0), (0, -1), (1, 0)], **kw):
        for face in (False, True):
            for rotate in (True, False):
                counts = {}
                want = self.model(table, counts=counts, face=face, rotate=rotate, **kw)
                assert not np.isnan(want).any()
                assert counts["occluded"] > 0, (what, "the pass changed nothing")
                assert_bit_equal(self.device(table, face=face, rotate=rotate, **kw), want, f"{what}, face={face}, rotate={rotate}")


# 5 x 7 and 1 x 40: frames smaller than the halo.  33 x 65: one pixel taller and one pixel wider than whole tiles of 32.
# 63 x 31: a partial tile in both directions and one that is all halo on the right.
@pytest.mark.parametrize("H,W", [(5, 7), (1, 40), (40, 1), (33, 65), (63, 31)])
def test_frames_that_do_not_fit_the_tiles(oracle, H, W):
    p = _Planes(oracle, H, W, seed=80 + H)
    p.check(f"{H} x {W}")
    R = 32
    far = [(R, R), (-R, -R), (R, 0), (0, -R), (3, 1), (-1, 2), (0, 1), (-1, 0)]
    p.check(f"{H} x {W}, halo 32", table=far, radius_px=R)
    if H > 8:
        p.check(f"{H} x {W}, rows 3 .. {H - 2}", y0=3, y1=H - 2)


def test_a_frame_of_more_tiles_than_the_grid_holds(oracle):
    """A launch is at most 2048 workgroups, each looping over tiles of 32 x 32: a frame 3 pixels wide and 65 600 tall is
    2050 tiles, so two workgroups make a second trip — 0.8 MB of z and winners, 2.4 MB each of colours and normals."""
    H, W = 65600, 3
    p = _Planes(oracle, H, W, seed=91)
    counts = {}
    table = [(0, 1), (1, -2), (-1, 3), (2, 0), (0, -5), (-2, -1), (1, 7), (0, -8)]
    want = p.model(table, counts=counts)
    assert counts["occluded"] > 1000 and (counts["ys"][counts["S"] > 0] >= 65536).any()      # the second trip's rows
    assert_bit_equal(p.device(table), want, "65600 x 3")


# ---- 3. random soups -----------------------------------------------------------------------------------------------

# (covered, occluded, pixels at the floor) from the host model
SOUP51 = {"plane": (34592, 29913, 1550), "face": (34592, 11626, 70)}
SOUP52 = {"plane": (253911, 208585, 13112), "face": (253911, 42730, 330)}


@pytest.mark.parametrize("seed,T,H,W,kw,presort,pinned", [
    (51, 4000, 200, 173, dict(size_px=(1.0, 40.0)), None, SOUP51),
    (52, 20000, 512, 509, dict(size_px=(2.0, 30.0)), True, SOUP52),
])
def test_random_soups(oracle, seed, T, H, W, kw, presort, pinned):
    s = _Scene(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), **kw), H, W)
    f = filler(H, W, presort=presort)
    for normals in ("plane", "face"):
        counts = {}
        s.check(f, f"soup{seed}, {normals}", counts=counts, normals=normals, **SOUP_KW)
        assert (counts["covered"], counts["occluded"], counts["at_floor"]) == pinned[normals]
        assert counts["occluded"] >= 0.05 * counts["covered"]
        assert counts["covered"] - counts["occluded"] >= 0.05 * counts["covered"]
        assert counts["at_floor"] > 0
    if presort:
        assert f._order is not None        # the resident inputs are the tile-coherent copies: the face mode went through d_pos_of


# ---- 4. special values, through the C entry ------------------------------------------------------------------------

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
    normal = p.normal.copy()
    hit = rng.uniform(size=(H, W)) < 0.1
    normal[hit] = rng.choice(np.float32([np.nan, 0.0, np.inf, -np.inf]), (int(hit.sum()), 3))
    normal[0, 0] = 0.0
    tri = p.tri.copy()
    tri[rng.uniform(size=tri.shape) < 0.05] = np.nan
    odd = dict(z=z, winner=winner, normal=normal, tri=tri)
    touched = 0
    for kw in (dict(), dict(rotate=False), dict(face=True), dict(face=True, rotate=False), dict(strength=50.0, floor=0.5),
               dict(min_cos=-1.0), dict(radius=1e30), dict(radius=1e-30), dict(radius_px=32)):
        counts = {}
        want = p.model(TABLE, counts=counts, T=T, **odd, **kw)
        assert not np.isnan(want).any()                  # every NaN fails `take`: none reaches the colours
        assert_bit_equal(p.device(TABLE, **odd, **kw), want, f"odd values, {kw}")
        touched = max(touched, counts["occluded"])
    assert touched > 300
    # an entry of d_pos_of beyond T: its pixels are not written in the face mode, and still occlude their neighbours
    perm = rng.permutation(T).astype(np.uint32)
    moved = np.empty_like(tri)
    moved[perm] = tri
    pos_of = perm.copy()
    gone = rng.uniform(size=T) < 0.3
    pos_of[gone] = rng.choice(np.uint32([T, T + 7, 2 ** 32 - 1]), int(gone.sum()))
    for rotate in (True, False):
        planes = dict(odd, tri=moved)
        want = p.model(TABLE, face=True, rotate=rotate, pos_of=pos_of, T=T, **planes)
        assert (want != p.color).any()
        assert_bit_equal(p.device(TABLE, face=True, rotate=rotate, pos_of=pos_of, **planes), want, "d_pos_of with entries beyond T")
        # the plane mode does not look at d_pos_of
        assert_bit_equal(p.device(TABLE, rotate=rotate, pos_of=pos_of, **planes), p.model(TABLE, rotate=rotate, T=T, **planes),
                         "the plane mode under a d_pos_of")
    # no triangles, and a frame that is background only: nothing is written
    assert_bit_equal(p.device(TABLE, T=0, **odd), p.color, "T == 0")
    assert_bit_equal(p.device(TABLE, **dict(odd, winner=np.full((H, W), -1, np.int32))), p.color, "background only")


# ---- 5. the filler -------------------------------------------------------------------------------------------------

def test_host_views_show_the_pass_and_their_edits_reach_it(soup256, filler256):
    s, f = soup256, filler256
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    f.ao_pass(**SOUP_KW)
    again = f.get_color_buffer()
    assert again is view
    want = s.want(**SOUP_KW)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(view, want, "after the pass")
    # an edit of the normals' host view reaches the pass
    s.draw(f)
    n = f.get_normals_buffer()
    n[:] = np.float32([0.0, 0.6, -0.8])
    f.ao_pass(**SOUP_KW)
    tilted = np.broadcast_to(np.float32([0.0, 0.6, -0.8]), s.cam.normals_buffer.shape)
    want_n = ao_ref.ao_pass(s.cam.color_buffer, s.cam.z_buffer, s.cam.winner, s.tri, s.cam.proj_mat, tilted, _table(SOUP_KW),
                            **_model_kw(SOUP_KW))
    assert (want_n != want).any()
    assert_bit_equal(f.get_color_buffer(), want_n, "under edited normals")
    # and one of the z view: a block pushed towards the eye occludes what surrounds it
    s.draw(f)
    zb = f.get_z_buffer()
    block = s.cam.z_buffer.copy()
    block[100:140, 100:140] = np.where(s.cam.winner[100:140, 100:140] >= 0, block[100:140, 100:140] - np.float32(2e-3),
                                       block[100:140, 100:140])
    zb[:] = block
    f.ao_pass(**SOUP_KW)
    want_z = ao_ref.ao_pass(s.cam.color_buffer, block, s.cam.winner, s.tri, s.cam.proj_mat, s.cam.normals_buffer,
                            _table(SOUP_KW), **_model_kw(SOUP_KW))
    assert (want_z != want).any()
    assert_bit_equal(f.get_color_buffer(), want_z, "under an edited z")
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
    kw = dict(normals="face", strength=1.0)
    want = s.want(**kw)
    assert (want != s.cam.color_buffer).any()
    f = filler(256, 256)                          # numpy
    s.draw(f)
    f.ao_pass(**kw)
    assert_bit_equal(host(f.get_color_tensor()), want, "numpy inputs")
    s.check_planes(f, "numpy inputs")
    f = filler(256, 256)                          # caller's device tensors
    f.render_arrays(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tri, col, nrm)], clear=True)
    f.ao_pass(**kw)
    assert_bit_equal(host(f.get_color_tensor()), want, "torch inputs")
    f = filler(256, 256)                          # the device-resident model
    f.render_model(DeviceModel(m), clear=True)
    f.ao_pass(**kw)
    assert_bit_equal(host(f.get_color_tensor()), want, "DeviceModel inputs")
    s.check_planes(f, "DeviceModel inputs")


# ---- 6. Renderer ---------------------------------------------------------------------------------------------------

AO = dict(radius=0.05, taps=16, strength=3.0, floor=0.25)


@pytest.mark.parametrize("on_device", [None, True, "fused"])
def test_renderer_with_guro_illumination(oracle, soup256, on_device):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    occluded = s.want(**AO)
    assert (occluded != s.cam.color_buffer).any()
    if on_device == "fused":
        # the raster kernel has shaded already: the pass multiplies what it stored
        want = s.want(color=oracle.guro(s.cam.color_buffer.copy(), s.cam.normals_buffer, GURO), **AO)
    else:
        want = oracle.guro(occluded.copy(), s.cam.normals_buffer, GURO)
    f = filler(256, 256)
    r = Renderer(f, GuroIllumination(GURO), on_device=on_device, ambient_occlusion=AO)
    for _ in range(2):                             # every frame starts from cleared buffers
        out = r.render(s.model)
        assert isinstance(out, np.ndarray) == (on_device is None)
        got = np.array(out) if on_device is None else host(out)
        assert np.array_equal(got, want)           # as values: the light leaves -0 on the background
        covered = s.cam.winner >= 0
        assert_bit_equal(got[covered], want[covered], f"Renderer(on_device={on_device!r}, ambient_occlusion=...)")
    s.check_planes(f, "after Renderer")
    plain = host(Renderer(filler(256, 256), GuroIllumination(GURO), on_device=True).render(s.model))
    assert (plain != want).any()


PHONG_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.25)]
PHONG_KW = dict(ambient=0.15, shininess=16)


def test_renderer_occludes_before_the_phong_pass(soup256):
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256

    def lit(color):
        return phong_ref.phong_pass(color, s.cam.winner, s.tri, s.cam.proj_mat, s.cam.normals_buffer, PHONG_LIGHTS, **PHONG_KW)
    want = lit(s.want(**AO))
    other = s.want(color=lit(s.cam.color_buffer), **AO)
    assert (want != other).any()                   # the two orders differ on this scene: the test can tell them apart
    f = filler(256, 256)
    r = Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, **PHONG_KW), on_device=True, ambient_occlusion=AO)
    got = host(r.render(s.model))
    assert_bit_equal(got, want, "Renderer(PhongIllumination, ambient_occlusion=...)")
    # and by hand
    a = filler(256, 256)
    s.draw(a)
    a.ao_pass(**AO)
    a.phong_pass(PHONG_LIGHTS, **PHONG_KW)
    assert_bit_equal(got, host(a.get_color_tensor()), "ao_pass, then phong_pass")
    s.check_planes(a, "ao_pass, then phong_pass")


def test_renderer_with_shadow_texture_and_supersampling(oracle, soup256):
    from cython3dmodelrenderer_amd import shadow
    from cython3dmodelrenderer_amd.data_structures.model import Model
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    occluded = s.want(**AO)
    # the shadow pass after the occlusion
    R, t = shadow_ref.rotation_frame(s.tri, (10, -20, 0))
    ltri, lnrm = shadow.light_arrays(s.tri, s.nrm, R, t)
    lig = oracle.OracleFiller(128, 160, fov=45.0)
    lig.render_arrays(ltri, s.col, lnrm)
    want = shadow_ref.shadow_pass(occluded, s.cam.winner, s.tri, s.cam.proj_mat, ltri, lig.proj_mat, lig.z_buffer, lig.winner,
                                  bias=2e-3, ambient=0.125, pcf=3)
    assert (want != occluded).any()
    f, g = filler(256, 256), filler(128, 160)
    r = Renderer(f, GuroIllumination(GURO), on_device="fused", ambient_occlusion=AO,
                 shadow=dict(filler=g, R=R, t=t, bias=2e-3, pcf=3, ambient=0.125))
    a, b = filler(256, 256), filler(128, 160)
    a.set_fused_illumination(GuroIllumination(GURO).light_direction)
    s.draw(a)
    b.render_arrays(ltri, s.col, lnrm, clear=True)
    a.bind_shadow_map(b, ltri)
    a.ao_pass(**AO)
    a.shadow_pass(bias=2e-3, pcf=3, ambient=0.125)
    assert_bit_equal(host(r.render(s.model)), host(a.get_color_tensor()), "ao_pass, then shadow_pass, under the fused light")
    a.set_fused_illumination(None)
    s.draw(a)
    a.ao_pass(**AO)
    a.shadow_pass(bias=2e-3, pcf=3, ambient=0.125)
    assert_bit_equal(host(a.get_color_tensor()), want, "ao_pass, then shadow_pass")
    # the texture pass before it
    rng = np.random.default_rng(72)
    T = len(s.tri)
    idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    uv = rng.uniform(0, 1, (T, 3, 2)).astype(np.float32)
    tex = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    m = Model(s.tri.reshape(-1, 3), idx, uv.reshape(-1, 2), idx, tex, s.nrm.reshape(-1, 3), idx, recalculate_normals=False)
    f = filler(256, 256)
    got = host(Renderer(f, GuroIllumination(GURO), on_device="fused", texture_pass={"perspective": True},
                         ambient_occlusion=AO).render(m))
    a = filler(256, 256)
    a.bind_texture(m.get_texture_coords_by_triangles(), tex)
    a.render_model(m, clear=True)
    a.texture_pass(perspective=True, light_direction=GuroIllumination(GURO).light_direction)
    textured = host(a.get_color_tensor())
    assert (textured != s.cam.color_buffer).any()
    assert_bit_equal(got, s.want(color=textured, **AO), "the texture with its light, then the occlusion")
    # supersampling: the pass runs on the supersampled frame, the resolve afterwards
    f = filler(256, 256)
    out = Renderer(f, GuroIllumination(GURO), None, 128, 128, on_device=True, supersample=2, ambient_occlusion=AO).render(s.model)
    assert tuple(out.shape) == (128, 128, 3)
    assert_bit_equal(host(f.get_color_tensor()), occluded, "the supersampled frame, occluded and unshaded")
    a = filler(256, 256)
    s.draw(a)
    a.ao_pass(**AO)
    assert_bit_equal(host(out), host(a.resolve(2, light_direction=GuroIllumination(GURO).light_direction)),
                     "Renderer(supersample=2, ambient_occlusion=...)")
    s.check_planes(f, "after the supersampled frame")


# ---- 7. errors -----------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(soup256):
    from cython3dmodelrenderer_amd import _capi
    s = soup256
    f = filler(256, 256, track_winner=False)
    s.draw(f)
    with pytest.raises(ValueError, match="winner plane"):
        f.ao_pass()
    f = filler(256, 256)
    with pytest.raises(ValueError, match="no frame has been rendered"):
        f.ao_pass()
    s.draw(f)
    f.render_arrays(s.tri, s.col, s.nrm)           # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.ao_pass()
    with pytest.raises(ValueError, match="swap chain"):
        filler(64, 64, pipeline=True).ao_pass()
    s.draw(f)
    with pytest.raises(ValueError, match="normals must be 'plane' or 'face', got 'vertex'"):
        f.ao_pass(normals="vertex")
    for bad in (0, 33, 8.0, True):
        with pytest.raises(ValueError, match="radius_px must be an int from 1 to 32"):
            f.ao_pass(radius_px=bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="taps must be a count from 1 to 64"):
            f.ao_pass(taps=bad)
    with pytest.raises(ValueError, match="taps must be a count from 1 to 64 or a list"):
        f.ao_pass(taps=[1, 2, 3])
    with pytest.raises(ValueError, match="taps must hold 1 to 64 pairs, got 0"):
        f.ao_pass(taps=[])
    with pytest.raises(ValueError, match="taps must hold 1 to 64 pairs, got 65"):
        f.ao_pass(taps=[(1, 0)] * 65)
    with pytest.raises(ValueError, match=r"the tap \(9, 0\) is \(0, 0\) or reaches beyond radius_px=8"):
        f.ao_pass(taps=[(1, 0), (9, 0)])
    with pytest.raises(ValueError, match=r"the tap \(0, 0\)"):
        f.ao_pass(taps=[(0, 0)])
    with pytest.raises(ValueError, match="9 taps do not fit radius_px=1"):
        f.ao_pass(taps=9, radius_px=1)
    with pytest.raises(_capi.CrenderError, match="radius is not finite and positive"):
        f.ao_pass(radius=0.0)
    with pytest.raises(_capi.CrenderError, match="not finite"):
        f.ao_pass(min_cos=float("nan"))
    with pytest.raises(_capi.CrenderError, match="strength is negative"):
        f.ao_pass(strength=-1.0)
    with pytest.raises(_capi.CrenderError, match="floor is not 0 .. 1"):
        f.ao_pass(floor=1.5)
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "nothing was written")
    f.ao_pass(**SOUP_KW)                           # and works again
    want = s.want(**SOUP_KW)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(host(f.get_color_tensor()), want, "after the errors")
    s.check_planes(f, "after the errors")


# ---- 8. bin overflow -----------------------------------------------------------------------------------------------

def test_a_frame_redrawn_after_a_bin_overflow_ends_occluded(oracle):
    """The scene of test_a_frame_redrawn_after_a_bin_overflow_ends_lit: the bin lists are far too small, the frame drops
    fragments and is rendered again when it is settled — which the pass does before it launches."""
    s = _Scene(oracle, random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0), 512, 512)
    kw = dict(radius=0.1, strength=3.0, normals="face")
    want = s.want(**kw)
    assert (want != s.cam.color_buffer).any()
    for more in (dict(), dict(presort=True)):
        f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False, **more)
        s.draw(f)
        need, cap = f.bin_usage()
        assert cap == 500 and need > cap and len(f._pending) == 1     # dropped fragments, nobody has looked yet
        f.ao_pass(**kw)
        assert not f._pending                                          # grown and redone before the pass
        assert_bit_equal(host(f.get_color_tensor()), want, f"a redone frame, {more}")
        s.check_planes(f, "a redone frame")
