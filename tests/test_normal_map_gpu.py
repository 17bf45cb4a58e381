"""Normal mapping on the GPU (csrc/normal_map.hip's k_nmap_shade and k_nmap_from_height through
AdvancedPixelBufferFiller.bind_normal_map / normal_map_pass, the C entries and Renderer), bit for bit against the host
model of tests/nmap_ref.py evaluated on the oracle's frames (itself pinned in tests/test_normal_map_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import mip_ref
import nmap_ref
import phong_ref
import tex_ref
from pass_scenes import LIGHT, Scene, filler, host, soup_fixture, soup_textured, texture, textured_model, trex_arrays, \
    trex_fixture, trex_textured
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu


def _maps():
    """64 x 64 from a height map; 37 x 53 of random bytes (odd, not square: the chain's clamped edges; bytes of 0: the
    clamp at -1; components that point into the surface); one texel."""
    rough = texture(9, 37, 53)
    rough[::5, ::3] = 0
    return {"64x64": nmap_ref.from_height(texture(8, 64, 64)[:, :, 0], 1.0), "37x53": rough,
            "1x1": np.uint8([[[90, 170, 230]]])}


MAPS = _maps()
CHAINS = {k: mip_ref.build_chain(m) for k, m in MAPS.items()}


class _Scene(Scene):
    uv = None

    def want(self, nmap, filter, perspective, strength=1.0, normals=None, chain=None, **kw):
        return nmap_ref.normal_map_pass(self.cam.normals_buffer if normals is None else normals, self.cam.winner, self.tri,
                                        self.cam.proj_mat, self.uv, nmap, perspective, filter, strength, chain=chain, **kw)

    def check_other_planes(self, f, what):
        assert_bit_equal(host(f.get_z_tensor()), self.cam.z_buffer, f"{what}: z")
        assert_bit_equal(host(f.get_color_tensor()), self.cam.color_buffer, f"{what}: colour")
        assert_bit_equal(host(f.get_winner_tensor()), self.cam.winner, f"{what}: winner")

    def check(self, f, name, filter, perspective, what, strength=1.0):
        f.bind_normal_map(MAPS[name], uv_by_triangles=self.uv, mipmaps=filter == "trilinear")
        self.draw(f)
        f.normal_map_pass(strength, perspective, filter)
        counts = {}
        want = self.want(MAPS[name], filter, perspective, strength, chain=CHAINS[name], counts=counts)
        assert counts["written"] > 0.9 * self.covered, what
        assert_bit_equal(host(f.get_normals_tensor()), want, f"{what}: normals")
        self.check_other_planes(f, what)
        return want


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


@pytest.fixture(scope="module")
def scenes256(trex256, soup256):
    trex256.uv = trex_textured()[3]
    soup256.uv = soup_textured(71, 3000, 256, size_px=(3.0, 50.0))[3]
    assert_bit_equal(soup_textured(71, 3000, 256, size_px=(3.0, 50.0))[0], soup256.tri, "the soup's triangles")
    return {"trex": trex256, "soup": soup256}


# ---- 6. the pass, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("perspective", [False, True])
@pytest.mark.parametrize("filter", nmap_ref.FILTERS)
@pytest.mark.parametrize("scene", ["trex", "soup"])
def test_every_instance_on_three_maps(scenes256, scene, filter, perspective):
    s = scenes256[scene]
    f = filler(256, 256)
    for name in MAPS:
        s.check(f, name, filter, perspective, f"{scene}256, {name}, {filter}, perspective={perspective}")


def test_strength_and_the_identities(scenes256):
    s = scenes256["trex"]
    f = filler(256, 256)
    s.check(f, "64x64", "bilinear", True, "strength 2.5", strength=2.5)
    s.check(f, "37x53", "trilinear", False, "strength -0.75", strength=-0.75)
    for name, strength in (("64x64", 0.0), ("flat", 1.0)):
        nmap = MAPS[name] if name in MAPS else np.broadcast_to(np.uint8(nmap_ref.FLAT), (4, 4, 3)).copy()
        f.bind_normal_map(nmap, uv_by_triangles=s.uv)
        s.draw(f)
        f.normal_map_pass(strength, filter="nearest")
        assert_bit_equal(host(f.get_normals_tensor()), s.cam.normals_buffer, f"{name}, strength {strength}: nothing is written")


def test_a_frame_of_70_by_45(oracle):
    s = _Scene(oracle, trex_arrays(), 70, 45)
    s.uv = trex_textured()[3]
    assert s.covered > 300
    f = filler(70, 45)
    for filter in nmap_ref.FILTERS:
        s.check(f, "37x53", filter, True, f"70 x 45, {filter}")


def test_a_row_strip_leaves_the_other_rows_alone(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    s.uv = trex_textured()[3]
    f = filler(200, 173, row_strip=(y0, y1))
    f.bind_normal_map(MAPS["64x64"], uv_by_triangles=s.uv, mipmaps=True)
    for filter in ("bilinear", "trilinear"):
        s.draw(f)
        f.synchronize()
        # rows outside the strip: normals to be kept, and winners that WOULD be perturbed if the pass looked at them
        f.normals_buffer[:y0] = 7.5
        f.normals_buffer[y1:] = -2.25
        f.winner_buffer[:y0] = 0
        f.winner_buffer[y1:] = 1
        f.normal_map_pass(filter=filter)
        got = host(f.get_normals_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        want = s.want(MAPS["64x64"], filter, True, y0=y0, y1=y1)
        assert (want[y0:y1].view(np.uint32) != s.cam.normals_buffer[y0:y1].view(np.uint32)).any()
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, {filter}")


def test_a_presorted_filler_goes_through_pos_of(scenes256):
    s = scenes256["soup"]
    f = filler(256, 256, presort=True)
    for filter in nmap_ref.FILTERS:
        s.check(f, "37x53", filter, True, f"presorted, {filter}")
    assert f._order is not None            # the resident inputs are the tile-coherent copies: the pass went through d_pos_of


# ---- 7. the map from a height map, and the chain -----------------------------------------------------------------------

@pytest.mark.parametrize("wrap", [False, True])
def test_from_height_on_the_device(wrap):
    import torch
    f = filler(16, 16)
    rng = np.random.default_rng(17)
    for shape, scale in (((64, 64), 1.0), ((37, 53), -6.5), ((1, 1), 3.0), ((1, 7), 40.0), ((300, 2), 0.25)):
        h = rng.integers(0, 256, shape, dtype=np.uint8)
        want = nmap_ref.from_height(h, scale, wrap)
        f.bind_normal_map(height=h, scale=scale, wrap=wrap)
        got = f.get_normal_map()
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == shape + (3,)
        assert np.array_equal(host(got), want), (shape, scale, wrap)
        f.bind_normal_map(height=torch.from_numpy(h).cuda(), scale=scale, wrap=wrap, mipmaps=True)      # a device tensor
        assert np.array_equal(host(f.get_normal_map()), want), (shape, scale, wrap)
        # the chain is the texture's: the box average of the bytes
        chain, levels, offsets = f._normal_map[2]
        packed = mip_ref.pack_chain(mip_ref.build_chain(want))
        assert levels == mip_ref.layout(*shape)[0] and offsets == mip_ref.layout(*shape)[1]
        assert np.array_equal(host(chain), packed), (shape, "chain")
    f.bind_normal_map()
    assert f.get_normal_map() is None


# ---- 8. hand-built planes through the C entry --------------------------------------------------------------------------

def _shade(lib, winner, tri, P, uv, nmap, mh, mw, normal, flags, strength=1.0, T=None, pos_of=None):
    import torch
    from cython3dmodelrenderer_amd import _capi
    T = tri.shape[0] if T is None else T
    H, W = winner.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.crender_nmap_shade(
        winner.data_ptr(), tri.data_ptr() if T else None, T, None if pos_of is None else pos_of.data_ptr(), _capi.f32_16(P),
        uv.data_ptr() if T else None, nmap.data_ptr(), mh, mw, strength, normal.data_ptr(), H, W, 0, H, flags, st),
        "crender_nmap_shade")
    return host(normal)


def test_special_values_through_the_c_entry(oracle):
    import torch
    from cython3dmodelrenderer_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(61)
    H, W, T = 40, 37, 300
    tri, col, nrm = random_soup(rng, T, 40, size_px=(3.0, 25.0))
    uv = rng.uniform(-1.5, 2.5, (T, 3, 2)).astype(np.float32)
    cam = oracle.OracleFiller(H, W, fov=45.0)
    cam.render_arrays(tri, col, nrm)
    assert (cam.winner >= 0).sum() > 500
    tri, normal, winner = tri.copy(), cam.normals_buffer.copy(), cam.winner.copy()
    # corners that are NaN, infinite, huge or zero; triangles of no area
    hit = rng.uniform(size=tri.shape) < 0.03
    tri[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0]), int(hit.sum()))
    flat = rng.uniform(size=T) < 0.05
    tri[flat, 1] = tri[flat, 0]
    line = rng.uniform(size=T) < 0.03
    with np.errstate(all="ignore"):                  # (some of these corners are the huge ones)
        tri[line, 2] = tri[line, 0] + (tri[line, 1] - tri[line, 0]) * np.float32(2)
    # uv: det = 0 (three equal pairs), det = NaN, infinite, far outside [0, 1]
    same = rng.uniform(size=T) < 0.08
    uv[same, 1] = uv[same, 2] = uv[same, 0]
    hit = rng.uniform(size=uv.shape) < 0.03
    uv[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 3e38, -1e13, 2147483648.0, 1e-42, 5e4]), int(hit.sum()))
    # a tangent exactly along the normal: Tt = (0.5, 0, 0) under the normal (1, 0, 0) at every pixel of a block
    along = 7
    tri[along] = np.float32([[-0.2, -0.2, 1.5], [0.3, -0.2, 1.5], [-0.2, 0.3, 1.5]])
    uv[along] = np.float32([[0, 0], [1, 0], [0, 1]])
    winner[8:16, 8:16] = along
    normal[8:16, 8:16] = np.float32([1.0, 0.0, 0.0])
    # normals that are zero, NaN or infinite; winners that name no triangle
    hit = (rng.uniform(size=(H, W)) < 0.1)
    hit[8:16, 8:16] = False
    normal[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0]), (int(hit.sum()), 3))
    hit = rng.uniform(size=winner.shape) < 0.1
    hit[8:16, 8:16] = False
    winner[hit] = rng.choice(np.int32([-1, -2, T, T + 1, 2 ** 31 - 1, -2 ** 31]), int(hit.sum()))
    assert {-1, T, 2 ** 31 - 1} <= set(np.unique(winner))
    name = "37x53"
    nmap, chain = MAPS[name], CHAINS[name]
    assert (nmap == 0).any()
    mh, mw = nmap.shape[:2]
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
           dict(winner=winner, tri=tri, uv=uv, nmap=nmap, chain=mip_ref.pack_chain(chain)).items()}

    def model(filter, perspective, w=winner, strength=1.0, counts=None):
        out = nmap_ref.normal_map_pass(normal, w, tri, cam.proj_mat, uv, nmap, perspective, filter, strength, chain=chain,
                                       counts=counts)
        written = (out.view(np.uint32) != normal.view(np.uint32)).any(2)
        assert not np.isnan(out[written]).any()          # no NaN is ever written
        return out

    def flags_of(filter, perspective):
        return (_capi.NMAP_PERSPECTIVE if perspective else 0) | {"nearest": 0, "bilinear": _capi.NMAP_BILINEAR,
                                                                 "trilinear": _capi.NMAP_CHAIN}[filter]
    for filter in nmap_ref.FILTERS:
        for perspective in (False, True):
            counts = {}
            want = model(filter, perspective, counts=counts)
            assert 300 < counts["written"] < counts["covered"] - 100 and counts["det_zero"] > 50
            assert not counts["mask"][8:16, 8:16].any()                       # the tangent along the normal: tl == 0
            got = _shade(lib, dev["winner"], dev["tri"], cam.proj_mat, dev["uv"], dev["chain" if filter == "trilinear" else "nmap"],
                         mh, mw, torch.from_numpy(normal).cuda(), flags_of(filter, perspective))
            assert_bit_equal(got, want, f"odd values, {filter}, perspective={perspective}")
    # an entry of d_pos_of beyond T makes its triangle background; the others are found where it says
    perm = rng.permutation(T).astype(np.uint32)
    moved = np.empty_like(tri)
    moved[perm] = tri
    pos_of = perm.copy()
    gone = rng.uniform(size=T) < 0.3
    pos_of[gone] = rng.choice(np.uint32([T, T + 7, 2 ** 32 - 1]), int(gone.sum()))
    masked = np.where((winner >= 0) & (winner < T) & gone[np.clip(winner, 0, T - 1)], -1, winner).astype(np.int32)
    got = _shade(lib, dev["winner"], torch.from_numpy(moved).cuda(), cam.proj_mat, dev["uv"], dev["chain"], mh, mw,
                 torch.from_numpy(normal).cuda(), flags_of("trilinear", True), strength=-1.5,
                 pos_of=torch.from_numpy(pos_of.view(np.int32)).cuda())
    assert_bit_equal(got, model("trilinear", True, masked, strength=-1.5), "d_pos_of with entries beyond T")
    # no triangles, and a frame that is background only: nothing is written
    for kw in (dict(T=0), dict()):
        w = dev["winner"] if kw else torch.full((H, W), -1, dtype=torch.int32).cuda()
        got = _shade(lib, w, dev["tri"], cam.proj_mat, dev["uv"], dev["nmap"], mh, mw, torch.from_numpy(normal).cuda(),
                     flags_of("bilinear", True), **kw)
        assert_bit_equal(got, normal, f"nothing to perturb, {kw}")


# ---- 9. downstream: everything that lights a pixel reads the plane -----------------------------------------------------

POINT = [dict(position=(-0.8, -0.5, -0.2), diffuse=0.9, specular=0.5)]


def test_phong_and_the_illumination_pass_see_the_bumps(oracle, scenes256):
    from cython3dmodelrenderer_amd.illumination.guro_illumination import GuroIllumination
    s = scenes256["trex"]
    bumped = s.want(MAPS["64x64"], "bilinear", True)
    f = filler(256, 256)
    f.bind_normal_map(MAPS["64x64"], uv_by_triangles=s.uv)
    s.draw(f)
    f.normal_map_pass()
    f.phong_pass(POINT)
    want = phong_ref.phong_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, bumped, POINT)
    smooth = phong_ref.phong_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.cam.normals_buffer, POINT)
    assert (want != smooth).any(2).sum() > 10000
    assert_bit_equal(host(f.get_color_tensor()), want, "phong_pass after normal_map_pass")
    assert_bit_equal(host(f.get_normals_tensor()), bumped, "the plane phong_pass read")
    s.draw(f)
    f.normal_map_pass()
    assert GuroIllumination(LIGHT).draw_illumination_device(f)
    want = oracle.guro(s.cam.color_buffer.copy(), bumped, LIGHT)
    assert (want != oracle.guro(s.cam.color_buffer.copy(), s.cam.normals_buffer, LIGHT)).any(2).sum() > 10000
    assert_bit_equal(host(f.get_color_tensor()), want, "the illumination pass after normal_map_pass")


@pytest.fixture(scope="module")
def model_frame(oracle):
    m, tex = textured_model()
    tri, col, nrm = m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles
    s = _Scene(oracle, (tri, col, nrm), 256, 256)
    s.uv = m.get_texture_coords_by_triangles()
    s.model, s.tex = m, tex
    assert s.covered > 10000
    return s


NMAP_OPTS = dict(strength=1.5, perspective=True, filter="trilinear")


@pytest.mark.parametrize("on_device", [None, False, True])
def test_renderer_with_a_normal_map(oracle, model_frame, on_device):
    from cython3dmodelrenderer_amd.illumination.guro_illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = model_frame
    bumped = s.want(MAPS["37x53"], "trilinear", True, 1.5, chain=CHAINS["37x53"])
    want = oracle.guro(s.cam.color_buffer.copy(), bumped, LIGHT)
    f = filler(256, 256)
    r = Renderer(f, GuroIllumination(LIGHT), on_device=on_device, normal_map=dict(normal_map=MAPS["37x53"], **NMAP_OPTS))
    for _ in range(2):                             # every frame starts from cleared buffers: the same image twice
        out = r.render(s.model)
        assert_bit_equal(host(out) if on_device is True else np.array(out), want, f"Renderer(on_device={on_device!r})")
    assert_bit_equal(host(f.get_normals_tensor()), bumped, "the normal plane after Renderer")
    if on_device is True:
        # the same chain by hand
        a = filler(256, 256)
        a.bind_normal_map(MAPS["37x53"], uv_by_triangles=s.uv, mipmaps=True)
        a.render_model(s.model, clear=True)
        a.normal_map_pass(**NMAP_OPTS)
        GuroIllumination(LIGHT).draw_illumination_device(a)
        assert_bit_equal(host(out), host(a.get_color_tensor()), "by hand")
        # the map from a height map, under supersampling: the pass runs on the supersampled frame, the resolve lights
        h = texture(4, 16, 16)[:, :, 0]
        out = Renderer(f, GuroIllumination(LIGHT), None, 128, 128, on_device=True, supersample=2,
                       normal_map=dict(height=h, scale=2.0, wrap=True, filter="nearest")).render(s.model)
        a.bind_normal_map(height=h, scale=2.0, wrap=True, uv_by_triangles=s.uv)
        a.render_model(s.model, clear=True)
        a.normal_map_pass(filter="nearest")
        light = [float(v) for v in oracle.guro_light(LIGHT)]
        assert_bit_equal(host(out), host(a.resolve(2, light_direction=light)), "Renderer(supersample=2, normal_map=...)")
        assert_bit_equal(host(a.get_normals_tensor()),
                         s.want(nmap_ref.from_height(h, 2.0, True), "nearest", True), "the supersampled frame's normals")


def test_renderer_fused_carries_the_light_in_the_texture_pass(oracle, model_frame):
    from cython3dmodelrenderer_amd.illumination.guro_illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = model_frame
    with pytest.raises(ValueError, match="without a texture_pass"):
        Renderer(filler(256, 256), GuroIllumination(LIGHT), on_device="fused", normal_map=dict(normal_map=MAPS["64x64"]))
    bumped = s.want(MAPS["64x64"], "bilinear", True)
    want = tex_ref.texture_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.uv, s.tex, True, True,
                                normals=bumped, light_direction=LIGHT)
    smooth = tex_ref.texture_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.uv, s.tex, True, True,
                                  normals=s.cam.normals_buffer, light_direction=LIGHT)
    assert (want != smooth).any(2).sum() > 10000
    r = Renderer(filler(256, 256), GuroIllumination(LIGHT), on_device="fused",
                 texture_pass={"perspective": True, "filter": "bilinear"}, normal_map=dict(normal_map=MAPS["64x64"]))
    for _ in range(2):
        assert_bit_equal(host(r.render(s.model)), want, "Renderer('fused', texture_pass, normal_map)")


def test_errors_name_their_cause(scenes256):
    from cython3dmodelrenderer_amd.data_structures.model import Model
    from cython3dmodelrenderer_amd.illumination.guro_illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = scenes256["soup"]
    nmap = MAPS["64x64"]
    chain = filler(64, 64, pipeline=True)
    chain.bind_normal_map(nmap, uv_by_triangles=s.uv)
    with pytest.raises(ValueError, match="swap chain"):
        chain.normal_map_pass()
    f = filler(256, 256, track_winner=False)
    f.bind_normal_map(nmap, uv_by_triangles=s.uv)
    s.draw(f)
    with pytest.raises(ValueError, match="winner plane"):
        f.normal_map_pass()
    f = filler(256, 256)
    with pytest.raises(ValueError, match="no normal map is bound"):
        f.normal_map_pass()
    f.bind_normal_map(nmap)
    with pytest.raises(ValueError, match="no texture coordinates are bound"):
        f.normal_map_pass()
    f.bind_texture(s.uv, texture(3, 8, 8))         # None: the uv of bind_texture at the time the pass runs
    with pytest.raises(ValueError, match="no frame has been rendered"):
        f.normal_map_pass()
    s.draw(f)
    with pytest.raises(ValueError, match="needs a mip chain"):
        f.normal_map_pass(filter="trilinear")
    with pytest.raises(ValueError, match="filter must be"):
        f.normal_map_pass(filter="cubic")
    with pytest.raises(ValueError, match="strength must be a finite number"):
        f.normal_map_pass(strength=float("nan"))
    f.normal_map_pass()
    assert_bit_equal(host(f.get_normals_tensor()), s.want(nmap, "bilinear", True), "the uv of bind_texture")
    f.bind_normal_map(nmap, uv_by_triangles=s.uv[:-1])
    s.draw(f)
    with pytest.raises(ValueError, match="2999 triangles of texture coordinates are bound, the last frame drew 3000"):
        f.normal_map_pass()
    f.render_arrays(s.tri, s.col, s.nrm)           # composites on the frame before
    f.bind_normal_map(nmap, uv_by_triangles=s.uv)
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.normal_map_pass()
    for bad in (dict(normal_map=nmap, height=nmap[..., 0]), dict(normal_map=nmap[..., 0]), dict(normal_map=nmap.astype(np.float32)),
                dict(normal_map=nmap[:, :, :2]), dict(height=nmap), dict(height=nmap[..., 0].astype(np.int32)),
                dict(normal_map=nmap, uv_by_triangles=s.uv.astype(np.float64)), dict(normal_map=nmap, uv_by_triangles=s.uv[:, :, :1]),
                dict(height=nmap[..., 0], scale=float("inf"))):
        with pytest.raises(ValueError):
            f.bind_normal_map(**bad)
    T = len(s.tri)
    idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    plain = Model(s.tri.reshape(-1, 3), idx, normals=s.nrm.reshape(-1, 3), triangles_normals=idx, recalculate_normals=False)
    plain.set_uniform_color()
    with pytest.raises(ValueError, match="texture coordinates"):
        Renderer(filler(64, 64), GuroIllumination(LIGHT), normal_map=dict(normal_map=nmap)).render(plain)


# ---- 10. host views ----------------------------------------------------------------------------------------------------

def test_host_views_show_the_new_normals_at_the_next_getter_call(scenes256):
    s = scenes256["soup"]
    nmap = MAPS["64x64"]
    f = filler(256, 256)
    f.bind_normal_map(nmap, uv_by_triangles=s.uv)
    s.draw(f)
    view = f.get_normals_buffer()
    assert_bit_equal(view, s.cam.normals_buffer, "before the pass")
    f.normal_map_pass()
    again = f.get_normals_buffer()
    assert again is view
    assert_bit_equal(view, s.want(nmap, "bilinear", True), "after the pass")
    # an edit of the view made before the pass is what the pass perturbs
    s.draw(f)
    n = f.get_normals_buffer()
    n[:] = np.float32([0.0, 0.0, -1.0])
    f.normal_map_pass()
    flat = np.broadcast_to(np.float32([0.0, 0.0, -1.0]), s.cam.normals_buffer.shape)
    want = s.want(nmap, "bilinear", True, normals=flat)
    assert (want != s.want(nmap, "bilinear", True)).any()
    assert_bit_equal(f.get_normals_buffer(), want, "under edited normals")
