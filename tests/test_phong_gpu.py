"""The deferred Phong pass on the GPU (csrc/phong.hip through AdvancedPixelBufferFiller.phong_pass, PhongIllumination
and Renderer), bit for bit against the host model of tests/phong_ref.py evaluated on the oracle's frames (itself
pinned on T-Rex in tests/test_phong_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import phong_ref
import shadow_ref
from pass_scenes import GOLDEN, Scene, filler, host, soup_fixture, trex_arrays, trex_fixture
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)              # what GuroIllumination is constructed with
POINT = (-0.8, -0.5, -0.2)
SECOND = (1.5, -2.0, -0.5)
ONE_POINT = [dict(position=POINT, diffuse=0.9, specular=0.5)]
ONE_DIRECTION = [dict(direction=GURO, diffuse=0.9, specular=0.5)]
FOUR = [dict(position=POINT, diffuse=0.6, specular=0.5), dict(direction=GURO, diffuse=0.3, specular=0.25),
        dict(position=SECOND, diffuse=0.0, specular=0.0), dict(direction=(-1.0, 0.5, 0.25), diffuse=0.2, specular=0.125)]
LIGHTS = {"point": ONE_POINT, "direction": ONE_DIRECTION, "four": FOUR}


class _Scene(Scene):
    def want(self, lights, color=None, **kw):
        out = phong_ref.phong_pass(self.cam.color_buffer if color is None else color, self.cam.winner, self.tri,
                                   self.cam.proj_mat, self.cam.normals_buffer, lights, **kw)
        assert not np.isnan(out).any()
        return out

    def check(self, f, lights, what, **kw):
        self.draw(f)
        f.phong_pass(lights, **kw)
        want = self.want(lights, **kw)
        self.assert_changed(want, what)
        assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour")
        self.check_planes(f, what)
        return want


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


# ---- 1. T-Rex ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shininess", [1, 32, 4096])
@pytest.mark.parametrize("kind", ["point", "direction", "four"])
def test_trex_every_instance(trex256, kind, shininess):
    s = trex256
    assert s.covered == 15801
    s.check(filler(256, 256), LIGHTS[kind], f"trex256, {kind}, shininess {shininess}", shininess=shininess)


def test_trex_other_coefficients(trex256):
    s = trex256
    f = filler(256, 256)
    s.check(f, ONE_POINT + [dict(position=SECOND, diffuse=0.9, specular=0.5)], "two points, no clamp",
            ambient=0.0, shininess=128, specular_color=(3.0, 200.0, 17.5), clamp=float("inf"))
    s.check(f, ONE_POINT, "clamp 100", ambient=0.25, shininess=2, clamp=100.0)


def test_one_directional_diffuse_light_is_guro(oracle, trex256):
    s = trex256
    f = filler(256, 256)
    s.draw(f)
    f.phong_pass([dict(direction=GURO, diffuse=1.0, specular=0.0)], ambient=0.0, clamp=float("inf"))
    got = host(f.get_color_tensor())
    want = oracle.guro(s.cam.color_buffer.copy(), s.cam.normals_buffer, GURO)
    covered = s.cam.winner >= 0
    assert np.array_equal(got[covered], want[covered])                       # as values: -0 against +0 is allowed
    assert_bit_equal(got[~covered], s.cam.color_buffer[~covered], "the background is not written")


# ---- 2. odd shapes -------------------------------------------------------------------------------------------------

def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_alone(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    for kind in ("point", "four"):
        s.draw(f)
        f.synchronize()
        # rows outside the strip: colours to be kept, and winners that WOULD be lit if the pass looked at them
        f.color_buffer[:y0] = 7.5
        f.color_buffer[y1:] = -2.25
        f.winner_buffer[:y0] = 0
        f.winner_buffer[y1:] = 1
        f.phong_pass(LIGHTS[kind])
        got = host(f.get_color_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        want = s.want(LIGHTS[kind], y0=y0, y1=y1)
        assert (want[y0:y1].view(np.uint32) != s.cam.color_buffer[y0:y1].view(np.uint32)).any()
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, {kind}")


# ---- 3. random soups -----------------------------------------------------------------------------------------------

# The first light stands INSIDE the soup's depth range (0.5 .. 3): the triangles in front of it have it behind them.
SOUP_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.25)]


# (the covered pixels, [(lit, unlit) under each of the two lights]) from the host model: 9.7 % and 91.8 % lit of soup 51,
# 24.3 % and 91.3 % of soup 52
SOUP51 = (34592, [(3361, 31231), (31745, 2847)])
SOUP52 = (253911, [(61694, 192217), (231812, 22099)])


@pytest.mark.parametrize("seed,T,H,W,kw,presort,counts", [
    (51, 4000, 200, 173, dict(size_px=(1.0, 40.0)), None, SOUP51),
    (52, 20000, 512, 509, dict(size_px=(2.0, 30.0)), True, SOUP52),
])
def test_random_soups(oracle, seed, T, H, W, kw, presort, counts):
    s = _Scene(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), **kw), H, W)
    got = {}
    s.want(SOUP_LIGHTS, counts=got)
    assert (got["covered"], [(l["lit"], l["unlit"]) for l in got["lights"]]) == counts
    for l in got["lights"]:
        assert min(l["lit"], l["unlit"]) >= 0.02 * got["covered"]
    f = filler(H, W, presort=presort)
    s.check(f, SOUP_LIGHTS, f"soup{seed}")
    s.check(f, SOUP_LIGHTS[:1], f"soup{seed}, one light", shininess=4)
    if presort:
        assert f._order is not None        # the resident inputs are the tile-coherent copies: the pass went through d_pos_of


# ---- 4. special values, through the C entry ------------------------------------------------------------------------

def _shade(lib, winner, tri, P, normal, lights, color, ambient=0.1, shininess=32, spec=(255.0, 255.0, 255.0), clamp=255.0,
           T=None, pos_of=None):
    import torch
    from cython3dmodelrenderer_amd import _capi
    T = tri.shape[0] if T is None else T
    H, W = winner.shape
    L5, mask = phong_ref.lights5(lights)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.crender_phong_shade(
        winner.data_ptr(), tri.data_ptr() if T else None, T, None if pos_of is None else pos_of.data_ptr(), _capi.f32_16(P),
        normal.data_ptr(), (C.c_float * L5.size)(*L5.reshape(-1).tolist()), len(lights), mask, ambient,
        int(shininess).bit_length() - 1, (C.c_float * 3)(*spec), clamp, color.data_ptr(), H, W, 0, H, 0, st),
        "crender_phong_shade")
    return host(color)


def test_special_values_through_the_c_entry(oracle):
    import torch
    from cython3dmodelrenderer_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(61)
    H, W, T = 40, 37, 300
    tri, col, nrm = random_soup(rng, T, 40, size_px=(3.0, 25.0))
    cam = oracle.OracleFiller(H, W, fov=45.0)
    cam.render_arrays(tri, col, nrm)
    assert (cam.winner >= 0).sum() > 500
    # corners that are NaN, infinite, huge or zero; normals that are NaN, infinite or zero; winners that name no triangle
    odd = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0])
    tri = tri.copy()
    hit = rng.uniform(size=tri.shape) < 0.05
    tri[hit] = rng.choice(odd, int(hit.sum()))
    normal = cam.normals_buffer.copy()
    hit = rng.uniform(size=(H, W)) < 0.1
    normal[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 0.0]), (int(hit.sum()), 3))
    bad = np.int32([-1, -2, T, T + 1, 2 ** 31 - 1, -2 ** 31])
    winner = cam.winner.copy()
    hit = rng.uniform(size=winner.shape) < 0.1
    winner[hit] = rng.choice(bad, int(hit.sum()))
    color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    # a light exactly on a vertex of a triangle that is seen, one at the origin (the eye: L = V everywhere), and a
    # direction
    seen = [int(t) for t in winner[(winner >= 0) & (winner < T)] if np.isfinite(tri[t]).all() and (tri[t] != 0).all()]
    vertex = [float(v) for v in tri[seen[0], 0]]
    lights = [dict(position=vertex, diffuse=0.7, specular=0.5), dict(position=(0.0, 0.0, 0.0), diffuse=0.4, specular=0.5),
              dict(direction=GURO, diffuse=0.3, specular=0.25)]

    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(winner=winner, tri=tri, normal=normal).items()}

    def model(w=winner, **kw):
        out = phong_ref.phong_pass(color, w, tri, cam.proj_mat, normal, kw.pop("lights", lights), **kw)
        assert not np.isnan(out).any()                   # every NaN is unlit: none reaches the colours
        return out
    touched = 0
    for kw in (dict(), dict(clamp=float("inf")), dict(clamp=100.0), dict(shininess=1), dict(shininess=4096, ambient=0.0),
               dict(lights=lights[:1]), dict(lights=lights[2:])):
        want = model(**kw)
        ckw = dict(kw)
        got = _shade(lib, dev["winner"], dev["tri"], cam.proj_mat, dev["normal"], ckw.pop("lights", lights),
                     torch.from_numpy(color).cuda(), **ckw)
        assert_bit_equal(got, want, f"odd values, {kw}")
        changed = int((want.view(np.uint32) != color.view(np.uint32)).any(2).sum())
        touched = max(touched, changed)
        if kw.get("clamp") == 100.0:
            assert want[(winner >= 0) & (winner < T)].max() == 100.0
    assert touched > 500
    # an entry of d_pos_of beyond T makes its triangle background; the others are found where it says
    perm = rng.permutation(T).astype(np.uint32)
    moved = np.empty_like(tri)
    moved[perm] = tri
    pos_of = perm.copy()
    gone = rng.uniform(size=T) < 0.3
    pos_of[gone] = rng.choice(np.uint32([T, T + 7, 2 ** 32 - 1]), int(gone.sum()))
    visible = np.where(winner >= 0, winner, 0)
    masked = np.where((winner >= 0) & (winner < T) & gone[np.clip(visible, 0, T - 1)], -1, winner).astype(np.int32)
    got = _shade(lib, dev["winner"], torch.from_numpy(moved).cuda(), cam.proj_mat, dev["normal"], lights,
                 torch.from_numpy(color).cuda(), pos_of=torch.from_numpy(pos_of.view(np.int32)).cuda())
    assert_bit_equal(got, model(masked), "d_pos_of with entries beyond T")
    # no triangles, and a frame that is background only: nothing is written
    for kw in (dict(T=0), dict()):
        w = dev["winner"] if kw else torch.full((H, W), -1, dtype=torch.int32).cuda()
        got = _shade(lib, w, dev["tri"], cam.proj_mat, dev["normal"], lights, torch.from_numpy(color).cuda(), **kw)
        assert_bit_equal(got, color, f"nothing to shade, {kw}")


# ---- 5. inputs -----------------------------------------------------------------------------------------------------

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
    want = s.want(FOUR)
    f = filler(256, 256)                          # numpy
    s.draw(f)
    f.phong_pass(FOUR)
    assert_bit_equal(host(f.get_color_tensor()), want, "numpy inputs")
    f = filler(256, 256)                          # caller's device tensors
    f.render_arrays(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tri, col, nrm)], clear=True)
    f.phong_pass(FOUR)
    assert_bit_equal(host(f.get_color_tensor()), want, "torch inputs")
    f = filler(256, 256)                          # the device-resident model
    f.render_model(DeviceModel(m), clear=True)
    f.phong_pass(FOUR)
    assert_bit_equal(host(f.get_color_tensor()), want, "DeviceModel inputs")


def test_host_views_show_the_lit_colours_at_the_next_getter_call(soup256):
    s = soup256
    f = filler(256, 256)
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    f.phong_pass(SOUP_LIGHTS)
    again = f.get_color_buffer()
    assert again is view
    assert_bit_equal(view, s.want(SOUP_LIGHTS), "after the pass")
    # an edit of the normals' host view reaches the pass
    s.draw(f)
    n = f.get_normals_buffer()
    n[:] = np.float32([0.0, 0.0, -1.0])
    f.phong_pass(SOUP_LIGHTS)
    flat = np.broadcast_to(np.float32([0.0, 0.0, -1.0]), s.cam.normals_buffer.shape)
    want = phong_ref.phong_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, flat, SOUP_LIGHTS)
    assert (want != s.want(SOUP_LIGHTS)).any()
    assert_bit_equal(f.get_color_buffer(), want, "under edited normals")


# ---- 6. Renderer ---------------------------------------------------------------------------------------------------

def _phong(**kw):
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    return PhongIllumination(lights=SOUP_LIGHTS, ambient=0.15, shininess=16, **kw)


PHONG_KW = dict(ambient=0.15, shininess=16)


@pytest.mark.parametrize("on_device", [None, True])
def test_renderer_renders_the_same_image_twice(soup256, on_device):
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    want = s.want(SOUP_LIGHTS, **PHONG_KW)
    f = filler(256, 256)
    r = Renderer(f, _phong(), on_device=on_device)
    for _ in range(2):                             # every frame starts from cleared buffers
        out = r.render(s.model)
        assert isinstance(out, np.ndarray) == (on_device is None)
        assert_bit_equal(np.array(out) if on_device is None else host(out), want, f"Renderer(on_device={on_device!r})")
    s.check_planes(f, "after Renderer")
    # one light through position=
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    out = Renderer(f, PhongIllumination(position=POINT), on_device=True).render(s.model)
    assert_bit_equal(host(out), s.want(ONE_POINT), "PhongIllumination(position=...)")


def test_renderer_with_a_texture_pass(soup256):
    from cython3dmodelrenderer_amd.data_structures.model import Model
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    rng = np.random.default_rng(72)
    T = len(s.tri)
    idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    uv = rng.uniform(0, 1, (T, 3, 2)).astype(np.float32)
    tex = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    m = Model(s.tri.reshape(-1, 3), idx, uv.reshape(-1, 2), idx, tex, s.nrm.reshape(-1, 3), idx, recalculate_normals=False)
    assert_bit_equal(m._vertices_by_triangles, s.tri, "the model's triangles")
    assert_bit_equal(m._normals_by_triangles, s.nrm, "the model's normals")
    f = filler(256, 256)
    got = host(Renderer(f, _phong(), on_device=True, texture_pass={"perspective": True}).render(m))
    a = filler(256, 256)
    a.bind_texture(m.get_texture_coords_by_triangles(), tex)
    a.render_model(m, clear=True)
    a.texture_pass(perspective=True)
    textured = host(a.get_color_tensor())
    assert (textured != s.cam.color_buffer).any()
    assert_bit_equal(got, s.want(SOUP_LIGHTS, color=textured, **PHONG_KW), "the texture unlit, then the light")


def test_renderer_casts_the_shadow_after_the_light(oracle, soup256):
    from cython3dmodelrenderer_amd import shadow
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    R, t = shadow_ref.rotation_frame(s.tri, (10, -20, 0))
    ltri, lnrm = shadow.light_arrays(s.tri, s.nrm, R, t)
    lig = oracle.OracleFiller(128, 160, fov=45.0)
    lig.render_arrays(ltri, s.col, lnrm)

    def shadowed(color):
        return shadow_ref.shadow_pass(color, s.cam.winner, s.tri, s.cam.proj_mat, ltri, lig.proj_mat, lig.z_buffer,
                                      lig.winner, bias=2e-3, ambient=0.125, pcf=3)
    want = shadowed(s.want(SOUP_LIGHTS, **PHONG_KW))
    other = s.want(SOUP_LIGHTS, color=shadowed(s.cam.color_buffer), **PHONG_KW)
    assert (want != other).any()                   # the two orders differ on this scene: the test can tell them apart
    f, g = filler(256, 256), filler(128, 160)
    r = Renderer(f, _phong(), on_device=True, shadow=dict(filler=g, R=R, t=t, bias=2e-3, pcf=3, ambient=0.125))
    got = host(r.render(s.model))
    assert_bit_equal(got, want, "Renderer(PhongIllumination, shadow=...)")
    # and by hand
    a, b = filler(256, 256), filler(128, 160)
    s.draw(a)
    b.render_arrays(ltri, s.col, lnrm, clear=True)
    a.bind_shadow_map(b, ltri)
    a.phong_pass(SOUP_LIGHTS, **PHONG_KW)
    a.shadow_pass(bias=2e-3, pcf=3, ambient=0.125)
    assert_bit_equal(got, host(a.get_color_tensor()), "phong_pass, then shadow_pass")


@pytest.mark.parametrize("on_device", [None, True])
def test_renderer_with_supersampling(soup256, on_device):
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    f = filler(256, 256)
    out = Renderer(f, _phong(), None, 128, 128, on_device=on_device, supersample=2).render(s.model)
    assert isinstance(out, np.ndarray) == (on_device is None)
    got = out if on_device is None else host(out)
    assert got.shape == (128, 128, 3)
    a = filler(256, 256)
    s.draw(a)
    a.phong_pass(SOUP_LIGHTS, **PHONG_KW)
    assert_bit_equal(host(a.get_color_tensor()), s.want(SOUP_LIGHTS, **PHONG_KW), "the supersampled frame, lit")
    assert_bit_equal(got, host(a.resolve(2)), "Renderer(supersample=2)")


# ---- 7. errors -----------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(soup256):
    from cython3dmodelrenderer_amd import _capi
    s = soup256
    f = filler(256, 256, track_winner=False)
    s.draw(f)
    with pytest.raises(ValueError, match="winner plane"):
        f.phong_pass(ONE_POINT)
    f = filler(256, 256)
    with pytest.raises(ValueError, match="no frame has been rendered"):
        f.phong_pass(ONE_POINT)
    s.draw(f)
    f.render_arrays(s.tri, s.col, s.nrm)           # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.phong_pass(ONE_POINT)
    with pytest.raises(ValueError, match="swap chain"):
        filler(64, 64, pipeline=True).phong_pass(ONE_POINT)
    s.draw(f)
    with pytest.raises(ValueError, match="1 to 4 dicts, got 0"):
        f.phong_pass([])
    with pytest.raises(ValueError, match="1 to 4 dicts, got 5"):
        f.phong_pass(ONE_POINT * 5)
    with pytest.raises(ValueError, match="exactly one of 'position' and 'direction'"):
        f.phong_pass([dict(position=POINT, direction=GURO, diffuse=1.0, specular=0.0)])
    with pytest.raises(ValueError, match="exactly one of 'position' and 'direction'"):
        f.phong_pass([dict(diffuse=1.0, specular=0.0)])
    with pytest.raises(ValueError, match="power of two from 1 to 4096, got 48"):
        f.phong_pass(ONE_POINT, shininess=48)
    with pytest.raises(_capi.CrenderError, match="not finite"):
        f.phong_pass(ONE_POINT, ambient=float("nan"))
    with pytest.raises(_capi.CrenderError, match="negative"):
        f.phong_pass([dict(position=POINT, diffuse=-1.0, specular=0.0)])
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "nothing was written")
    f.phong_pass(ONE_POINT)                        # and works again
    assert_bit_equal(host(f.get_color_tensor()), s.want(ONE_POINT), "after the errors")


# ---- 8. bin overflow -----------------------------------------------------------------------------------------------

def test_a_frame_redrawn_after_a_bin_overflow_ends_lit(oracle):
    """The scene of test_filler_recovers_from_bin_overflow: the bin lists are far too small, the frame drops fragments
    and is rendered again when it is settled — which the pass does before it launches."""
    s = _Scene(oracle, random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0), 512, 512)
    want = s.want(SOUP_LIGHTS)
    for kw in (dict(), dict(presort=True)):
        f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False, **kw)
        s.draw(f)
        need, cap = f.bin_usage()
        assert cap == 500 and need > cap and len(f._pending) == 1     # dropped fragments, nobody has looked yet
        f.phong_pass(SOUP_LIGHTS)
        assert not f._pending                                          # grown and redone before the pass
        assert_bit_equal(host(f.get_color_tensor()), want, f"a redone frame, {kw}")
        s.check_planes(f, "a redone frame")
