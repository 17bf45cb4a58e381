"""The environment pass on the GPU (k_env_shade of csrc/envmap.hip through AdvancedPixelBufferFiller.environment_pass,
the C entry and Renderer), bit for bit against the host model of tests/env_ref.py evaluated on the oracle's frames
(itself pinned in tests/test_env_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import env_ref
import pass_edges as E
from pass_scenes import Scene, Soup, filler, host, stream, trex_arrays, trex_fixture
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)              # what GuroIllumination is constructed with
TINT = (0.9, 0.5, 1.25)
KINDS = {"reflect": dict(), "background": dict(reflectivity=0.0, background=0.75), "both": dict(background=True)}


def _tilted():
    """The orientation whose z axis — where the camera looks — is (1, 1, 1) / sqrt 3 of the cube's frame."""
    z = np.ones(3) / np.sqrt(3.0)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1).astype(np.float32)


def _cube(seed=5, S=8):
    return np.random.default_rng(seed).integers(0, 256, (6, S, S, 3), dtype=np.uint8)


def _model_kw(kw):
    """environment_pass's arguments as env_ref.env_pass takes them: the background is None or the gain."""
    kw = dict(kw)
    b = kw.pop("background", None)
    kw["background"] = None if b is None or b is False else (1.0 if b is True else float(b))
    return kw


class _Scene(Scene):
    def want(self, levels, color=None, **kw):
        out = env_ref.env_pass(self.cam.color_buffer if color is None else color, self.cam.winner, self.tri,
                               self.cam.proj_mat, self.cam.normals_buffer, levels, **_model_kw(kw))
        assert not np.isnan(out).any()
        return out

    def check(self, f, levels, what, **kw):
        """Draws, runs the pass on the cube `f` has bound and compares; `levels` is what the model reads."""
        self.draw(f)
        f.environment_pass(**kw)
        want = self.want(levels, **{k: v for k, v in kw.items()})
        self.assert_changed(want, what)
        assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour")
        self.check_planes(f, what)
        return want


trex256 = trex_fixture(_Scene)


# ---- 1. T-Rex ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0.0, 0.5, 2.25])
@pytest.mark.parametrize("kind", list(KINDS))
def test_trex_every_instance(trex256, kind, level):
    """The six instances: with and without either flag, one level and two.  A side of 8 under a chain makes most samples
    touch a clamped face edge."""
    s = trex256
    assert s.covered == 15801
    cube = _cube()
    f = filler(256, 256)
    f.bind_environment(cube, mipmaps=True)
    assert f.environment_levels() == [8, 4, 2, 1]
    want = s.check(f, env_ref.chain_levels(cube), f"trex256, {kind}, level {level}", level=level, **KINDS[kind])
    covered = s.cam.winner >= 0
    if kind == "reflect":
        assert_bit_equal(want[~covered], s.cam.color_buffer[~covered], "the background is not written")
    if kind == "background":
        assert_bit_equal(want[covered], s.cam.color_buffer[covered], "the covered pixels are not written")


def test_the_chain_on_the_device_is_the_models(trex256):
    cube = _cube(seed=6, S=16)
    f = filler(64, 64)
    f.bind_environment(cube, mipmaps=True)
    assert_bit_equal(host(f.get_environment()), cube, "the cube")
    levels = env_ref.chain_levels(cube)
    assert f.environment_levels() == [16, 8, 4, 2, 1] == [l.shape[1] for l in levels]
    for j, want in enumerate(levels):
        assert_bit_equal(host(f.get_environment_level(j)), want, f"level {j}")
    f.bind_environment(cube)
    assert f.environment_levels() == [16] and f.get_environment_level(0) is f.get_environment()
    f.bind_environment(None)
    assert f.get_environment() is None and f.environment_levels() is None


def test_trex_other_operands(trex256):
    s = trex256
    f = filler(256, 256)
    one = _cube(seed=7, S=1)
    f.bind_environment(one)                       # a side of 1: every index is clamped to 0
    s.check(f, one, "S = 1", background=True)
    cube = _cube(seed=8, S=8)
    f.bind_environment(cube, mipmaps=True)
    levels = env_ref.chain_levels(cube)
    s.check(f, levels, "an orientation, a tint and f0", orientation=_tilted(), tint=TINT, f0=0.35, reflectivity=0.8,
            background=2.0, level=1.25)
    s.check(f, levels, "a mirror at the last level", f0=1.0, level=3)
    odd = _cube(seed=9, S=5)                      # a side that is no power of two, without a chain
    f.bind_environment(odd)
    s.check(f, odd, "S = 5", orientation=np.diag([-1.0, 1.0, -1.0]), background=True)
    # a device tensor binds like a numpy array
    import torch
    f.bind_environment(torch.from_numpy(cube).cuda(), mipmaps=True)
    s.check(f, levels, "a device tensor", level=0.5)


def test_the_sky_is_the_right_way_up(trex256):
    from cython3dmodelrenderer_amd.environment import gradient_sky
    s = trex256
    sky = gradient_sky(64, zenith=(10, 20, 250), horizon=(200, 200, 200), ground=(90, 60, 30))
    f = filler(256, 256)
    f.bind_environment(sky)
    want = s.check(f, sky, "a sky behind T-Rex", reflectivity=0.0, background=True)
    bg = s.cam.winner < 0
    assert bg[0].all() and bg[255].all()
    assert want[0, :, 2].min() > want[255, :, 2].max()          # blue falls down the frame: the upper rows look up


# ---- 2. odd shapes -------------------------------------------------------------------------------------------------

def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_alone(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    cube = _cube()
    f.bind_environment(cube, mipmaps=True)
    levels = env_ref.chain_levels(cube)
    for kw in (dict(), dict(background=True, level=0.5)):
        s.draw(f)
        f.synchronize()
        # rows outside the strip: colours to be kept, and winners that WOULD be shaded if the pass looked at them
        f.color_buffer[:y0] = 7.5
        f.color_buffer[y1:] = -2.25
        f.winner_buffer[:y0] = 0
        f.winner_buffer[y1:] = -1
        f.environment_pass(**kw)
        got = host(f.get_color_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        want = s.want(levels, y0=y0, y1=y1, **kw)
        assert (want[y0:y1].view(np.uint32) != s.cam.color_buffer[y0:y1].view(np.uint32)).any()
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, {kw}")


# ---- 3. random soups -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,T,H,W,kw,presort,covered", [
    (51, 4000, 200, 173, dict(size_px=(1.0, 40.0)), None, 34592),
    (52, 20000, 512, 509, dict(size_px=(2.0, 30.0)), True, 253911),
])
def test_random_soups(oracle, seed, T, H, W, kw, presort, covered):
    s = _Scene(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), **kw), H, W)
    cube = _cube(seed)
    levels = env_ref.chain_levels(cube)
    counts = {}
    env_ref.env_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.cam.normals_buffer, levels, counts=counts)
    assert counts["covered"] == covered == counts["written"] and min(counts["faces"]) >= 0.02 * covered
    f = filler(H, W, presort=presort)
    f.bind_environment(cube, mipmaps=True)
    s.check(f, levels, f"soup{seed}", orientation=_tilted(), background=True, tint=TINT)
    s.check(f, levels, f"soup{seed}, two levels", level=1.5, f0=0.5)
    if presort:
        assert f._order is not None        # the resident inputs are the tile-coherent copies: the pass went through d_pos_of


# ---- 4. special values, through the C entry ------------------------------------------------------------------------

def _shade(lib, winner, tri, P, normal, color, levels, level=0.0, orientation=None, reflectivity=1.0, f0=0.04,
           tint=(1.0, 1.0, 1.0), background=None, reflect=True, T=None, pos_of=None, y0=0, y1=None):
    """crender_env_shade on device tensors, with the model's arguments; -> the colour plane on the host."""
    import torch
    from cython3dmodelrenderer_amd import _capi
    T = tri.shape[0] if T is None else T
    H, W = winner.shape
    faces0, faces1, f = env_ref.pick_levels(levels if isinstance(levels, list) else [levels], level)
    d0 = torch.from_numpy(np.ascontiguousarray(faces0)).cuda()
    d1 = None if faces1 is None else torch.from_numpy(np.ascontiguousarray(faces1)).cuda()
    M = np.eye(3, dtype=np.float32) if orientation is None else np.asarray(orientation, np.float32)
    flags = (_capi.ENV_REFLECT if reflect else 0) | (_capi.ENV_BACKGROUND if background is not None else 0)
    _capi.check(lib.crender_env_shade(
        winner.data_ptr(), tri.data_ptr() if T else None, T, None if pos_of is None else pos_of.data_ptr(), _capi.f32_16(P),
        normal.data_ptr(), d0.data_ptr(), faces0.shape[1], None if d1 is None else d1.data_ptr(),
        0 if faces1 is None else faces1.shape[1], float(f), (C.c_float * 9)(*[float(v) for v in M.reshape(9)]),
        float(reflectivity), float(f0), (C.c_float * 3)(*[float(v) for v in tint]),
        0.0 if background is None else float(background), color.data_ptr(), H, W, y0, H if y1 is None else y1, flags, stream()),
        "crender_env_shade")
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
    cube = _cube(seed=61)
    levels = env_ref.chain_levels(cube)
    zero_row = np.float32([[0.6, 0.0, 0.8], [0.0, 0.0, 0.0], [-0.8, 0.0, 0.6]])      # d1 = 0: the faces +-y are never read

    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(winner=winner, tri=tri, normal=normal).items()}

    def model(w=winner, **kw):
        counts = {}
        out = env_ref.env_pass(color, w, tri, cam.proj_mat, normal, levels, counts=counts, **kw)
        assert not np.isnan(out).any()                   # a NaN is not usable or makes m a NaN: none reaches the colours
        return out, counts
    touched = 0
    for kw in (dict(), dict(orientation=zero_row), dict(orientation=zero_row, background=1.0, level=0.5),
               dict(background=0.5, reflect=False), dict(level=2.25, f0=1.0, tint=TINT), dict(reflectivity=0.0, background=1.0),
               dict(orientation=np.zeros((3, 3), np.float32), background=1.0)):
        want, counts = model(**kw)
        got = _shade(lib, dev["winner"], dev["tri"], cam.proj_mat, dev["normal"], torch.from_numpy(color).cuda(), levels, **kw)
        assert_bit_equal(got, want, f"odd values, {kw}")
        changed = int((want.view(np.uint32) != color.view(np.uint32)).any(2).sum())
        if kw.get("orientation") is not None and not np.any(kw["orientation"]):
            assert changed == 0                          # no direction is usable: nothing is written
        elif "orientation" in kw:
            assert counts["faces"][2] == counts["faces"][3] == 0
        if not kw:
            assert 0 < counts["written"] < counts["covered"]     # some pixels have no usable direction or weight
        touched = max(touched, changed)
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
    for kw in (dict(), dict(background=1.0)):
        got = _shade(lib, dev["winner"], torch.from_numpy(moved).cuda(), cam.proj_mat, dev["normal"], torch.from_numpy(color).cuda(),
                     levels, pos_of=torch.from_numpy(pos_of.view(np.int32)).cuda(), **kw)
        assert_bit_equal(got, model(masked, **kw)[0], f"d_pos_of with entries beyond T, {kw}")
    # no triangles, and a frame that is background only: a reflection writes nothing, a background every pixel
    empty = np.full((H, W), -1, np.int32)
    for kw in (dict(T=0), dict()):
        w = dev["winner"] if kw else torch.from_numpy(empty).cuda()
        got = _shade(lib, w, dev["tri"], cam.proj_mat, dev["normal"], torch.from_numpy(color).cuda(), levels, **kw)
        assert_bit_equal(got, color, f"nothing to mirror, {kw}")
        got = _shade(lib, w, dev["tri"], cam.proj_mat, dev["normal"], torch.from_numpy(color).cuda(), levels, background=1.0, **kw)
        want, counts = model(empty, background=1.0)
        assert counts["background"] == H * W == sum(counts["background_faces"])
        assert_bit_equal(got, want, f"a background alone, {kw}")


# ---- 5. a frame taller than a grid ---------------------------------------------------------------------------------

def test_the_tall_frame_through_the_c_entry(oracle):
    """tests/pass_edges.py's frame of 65 537 row blocks, two more than a grid may be tall: the rows of the loop's second trip
    are shaded, and by the same statements."""
    import torch
    from cython3dmodelrenderer_amd import _capi
    lib = _capi.load()
    s = E.tall_scene()
    y0 = E.TALL_Y0
    cube = _cube(seed=62)
    levels = env_ref.chain_levels(cube)
    kw = dict(level=0.5, orientation=_tilted(), background=1.0, f0=0.3)
    want = env_ref.env_pass(s.color, s.winner, s.tri, E.P, s.normals, levels, y0=y0, **kw)
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (s.winner, s.tri, s.normals, s.color)]
    got = _shade(lib, dev[0], dev[1], E.P, dev[2], dev[3], levels, y0=y0, **kw)
    assert_bit_equal(got[:y0], s.color[:y0], "tall frame: rows above y0")
    last = slice(E.TALL_H - 16, E.TALL_H)
    covered = (s.winner[last] >= 0) & (s.winner[last] < s.T)
    assert covered.any() and (~covered).any()
    assert (want[last].view(np.uint32) != s.color[last].view(np.uint32)).any(2).all(), "the second trip's rows change"
    assert_bit_equal(got[last], want[last], "tall frame: the second trip's rows")
    assert_bit_equal(got, want, "tall frame")
    assert_bit_equal(host(dev[0]), s.winner, "the winner plane is only read")
    assert_bit_equal(host(dev[2]), s.normals, "the normal plane is only read")


# ---- 6. Renderer ---------------------------------------------------------------------------------------------------

SIDE = 128
ENV = dict(level=0.5, f0=0.3, tint=TINT, background=True)
PHONG_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.25)]


@pytest.fixture(scope="module")
def small():
    return Soup(seed=73, T=800, res=SIDE)


def _hand(f, model, light, cube):
    """The documented order on the filler `f`: the cleared draw, the light in the form `light` names, the environment."""
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    f.bind_environment(cube, mipmaps=True)
    guro = GuroIllumination(GURO)
    if light == "fused":
        guro.fuse_into(f)
    f.render_model(model, clear=True)
    if light == "device":
        assert guro.draw_illumination_device(f)
    elif light == "host":
        guro.draw_illumination(f.get_color_buffer(), f.get_normals_buffer())
    elif light == "phong":
        f.phong_pass(PHONG_LIGHTS, ambient=0.15, shininess=16)
    f.environment_pass(**ENV)
    return f


@pytest.mark.parametrize("on_device,light", [(True, "device"), (None, "device"), (False, "host"), ("fused", "fused")])
def test_renderer_runs_the_pass_after_the_light(small, on_device, light):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    cube = _cube(seed=63)
    f = filler(SIDE, SIDE)
    r = Renderer(f, GuroIllumination(GURO), None, SIDE, SIDE, on_device=on_device, environment=dict(faces=cube, **ENV))
    assert f.environment_levels() == [8, 4, 2, 1]          # bound at construction, with the chain `level` needs
    want = host(_hand(filler(SIDE, SIDE), small, light, cube).get_color_tensor())
    plain = filler(SIDE, SIDE)
    plain.render_model(small, clear=True)
    assert (want != host(plain.get_color_tensor())).any(2).all()       # the background too: every pixel is shaded or painted
    for _ in range(2):                             # every frame starts from cleared buffers
        out = r.render(small)
        assert isinstance(out, np.ndarray) == (on_device in (None, False))
        assert_bit_equal(np.array(out) if isinstance(out, np.ndarray) else host(out), want, f"Renderer(on_device={on_device!r})")
    # the light first: the other order is another image
    other = filler(SIDE, SIDE)
    other.bind_environment(cube, mipmaps=True)
    other.render_model(small, clear=True)
    other.environment_pass(**ENV)
    GuroIllumination(GURO).draw_illumination_device(other)
    assert (host(other.get_color_tensor()) != want).any()


def test_renderer_with_a_phong_illumination(small):
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    cube = _cube(seed=63)
    f = filler(SIDE, SIDE)
    r = Renderer(f, PhongIllumination(lights=PHONG_LIGHTS, ambient=0.15, shininess=16), on_device=True,
                 environment=dict(faces=cube, **ENV))
    want = host(_hand(filler(SIDE, SIDE), small, "phong", cube).get_color_tensor())
    assert_bit_equal(host(r.render(small)), want, "Renderer(PhongIllumination, environment=...)")


@pytest.mark.parametrize("on_device", [True, None, False, "fused"])
def test_renderer_with_supersampling(small, on_device):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    cube = _cube(seed=63)
    f = filler(SIDE, SIDE)
    out = Renderer(f, GuroIllumination(GURO), None, SIDE // 2, SIDE // 2, on_device=on_device, supersample=2,
                   environment=dict(faces=cube, **ENV)).render(small)
    got = out if isinstance(out, np.ndarray) else host(out)
    assert got.shape == (SIDE // 2, SIDE // 2, 3)
    light = {True: "device", None: "device", False: "host", "fused": "fused"}[on_device]
    a = _hand(filler(SIDE, SIDE), small, light, cube)
    assert_bit_equal(got, host(a.resolve(2)), f"Renderer(supersample=2, on_device={on_device!r})")


@pytest.mark.parametrize("antialias", [False, True])
def test_renderer_draws_the_lines_after_the_pass(small, antialias):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    cube = _cube(seed=63)
    f = filler(SIDE, SIDE)
    more = dict(antialias={}) if antialias else {}
    out = Renderer(f, GuroIllumination(GURO), None, SIDE, SIDE, on_device=True, wireframe={},
                   environment=dict(faces=cube, **ENV), **more).render(small)
    a = _hand(filler(SIDE, SIDE), small, "device", cube)
    before = host(a.get_color_tensor()).copy()
    a.wire_pass()
    lined = host(a.get_color_tensor())
    assert (lined != before).any()
    assert_bit_equal(host(out), host(a.edge_aa()) if antialias else lined, f"wireframe, antialias={antialias}")
    if antialias:
        assert (host(out) != lined).any()


# ---- 7. errors -----------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(small):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    cube = _cube()
    f = filler(SIDE, SIDE)
    f.render_model(small, clear=True)
    with pytest.raises(ValueError, match="no environment is bound"):
        f.environment_pass()
    f.bind_environment(cube)
    with pytest.raises(ValueError, match="needs a mip chain"):
        f.environment_pass(level=0.5)
    with pytest.raises(ValueError, match="power of two, got 5"):
        f.bind_environment(_cube(S=5), mipmaps=True)
    for bad in (cube[:5], cube.astype(np.float32), cube[:, :, :4], cube[..., :2]):
        with pytest.raises(ValueError, match=r"faces must be uint8 \[6, S, S, 3\]"):
            f.bind_environment(bad)
    f.bind_environment(cube, mipmaps=True)
    with pytest.raises(ValueError, match="at most 3, the last level"):
        f.environment_pass(level=3.5)
    for kw, text in ((dict(reflectivity=1.5), "reflectivity must be"), (dict(f0=-0.1), "f0 must be"),
                     (dict(tint=(1.0, float("nan"), 1.0)), "tint must be"), (dict(tint=(1.0, 1.0)), "tint must be"),
                     (dict(level=-1.0), "level must be"), (dict(orientation=np.eye(4)), "orientation must be"),
                     (dict(orientation=np.full((3, 3), np.inf)), "orientation must be"), (dict(background=-1.0), "background must be"),
                     (dict(background="sky"), "background must be")):
        with pytest.raises(ValueError, match=text):
            f.environment_pass(**kw)
    before = host(f.get_color_tensor()).copy()
    f.environment_pass(reflectivity=0.0)           # nothing to do: no launch
    assert_bit_equal(host(f.get_color_tensor()), before, "nothing was written")
    with pytest.raises(ValueError, match="swap chain"):
        g = filler(64, 64, pipeline=True)
        g.bind_environment(cube)
        g.environment_pass()
    g = filler(SIDE, SIDE, track_winner=False)
    g.bind_environment(cube)
    g.render_model(small, clear=True)
    with pytest.raises(ValueError, match="winner plane"):
        g.environment_pass()
    g = filler(SIDE, SIDE)
    g.bind_environment(cube)
    with pytest.raises(ValueError, match="no frame has been rendered"):
        g.environment_pass()
    g.render_model(small, clear=True)
    g.render_model(small)                          # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        g.environment_pass()
    with pytest.raises(ValueError, match="swap chain"):
        Renderer(filler(64, 64, pipeline=True), GuroIllumination(GURO), on_device=True, environment=dict(faces=cube)).render(small)
    f.environment_pass()                           # and works again
    assert (host(f.get_color_tensor()) != before).any()
