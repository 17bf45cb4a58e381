"""The outline on the GPU (csrc/wireframe.hip's k_wire_outline through AdvancedPixelBufferFiller.wire_pass(outline=True)
and Renderer(wireframe=...)), bit for bit against the host model of tests/outline_ref.py evaluated on the oracle's
frames (itself pinned in tests/test_wire_outline_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import outline_ref
import overlay_ref
import phong_ref
import shadow_ref
from pass_scenes import GOLDEN, Scene, edge_mask, filler, host, soup_fixture, trex_arrays, trex_fixture
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)              # what GuroIllumination is constructed with
LINE = (250.0, 240.0, 20.0)
FILL = (30.0, 35.0, 40.0)


class _Scene(Scene):
    """The model's distance fields are kept by (mask, radius, bias, rows): they do not depend on the line's style."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self._fields = {}

    def want(self, base=None, mask_key=None, **kw):
        """The model's frame after ``wire_pass(outline=True, **kw)`` over `base` (the oracle's colours if None).
        `mask_key` names the edge mask for the cache of fields (None: no cache)."""
        kw = dict(kw)
        kw.pop("outline", None)
        kw["line"] = kw.pop("color", (255, 255, 255))
        r = kw.pop("radius_px", None)
        r = outline_ref.default_radius(kw.get("width", 1.0), kw.get("feather", 1.0)) if r is None else r
        bias = kw.pop("depth_bias", 1e-3)
        key = (mask_key, r, bias, kw.get("y0", 0), kw.get("y1"))
        field = self._fields.get(key) if mask_key is not None else None
        if field is None:
            field = outline_ref.distances(self.cam.winner, self.cam.z_buffer, self.tri, self.cam.proj_mat, kw.get("edges"), r,
                                          bias, kw.get("y0", 0), kw.get("y1"))
            if mask_key is not None:
                self._fields[key] = field
        return outline_ref.wire_pass(self.cam.color_buffer if base is None else base, self.cam.winner, self.cam.z_buffer,
                                     self.tri, self.cam.proj_mat, field=field, **kw)

    def check(self, f, what, mask_key=None, **kw):
        self.draw(f)
        f.wire_pass(outline=True, **kw)
        want = self.want(mask_key=mask_key, **kw)
        changed = self.assert_changed(want, what)
        assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour")
        self.check_planes(f, what)
        return want, changed


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


# ---- 1. T-Rex ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edges", ["all", "feature"])
@pytest.mark.parametrize("fill", [None, FILL])
def test_trex_every_instance(trex256, fill, edges):
    s = trex256
    assert s.covered == 15801
    f = filler(256, 256)
    mask = edge_mask(edges, s.tri)
    background = s.cam.winner < 0
    for radius_px in (1, 2, 8):
        for width in (1.0, 3.0):
            what = f"trex256, fill {fill}, {edges} edges, radius {radius_px}, width {width}"
            want, changed = s.check(f, what, mask_key=edges, color=LINE, fill=fill, edges=mask, radius_px=radius_px, width=width)
            assert (changed & background).any(), (what, "no background pixel changed")
            half = overlay_ref.wire_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, width=width, line=LINE,
                                         fill=fill, edges=mask)
            assert (want != half).any(), (what, "the same as outline=False")


# ---- 2. the edges of the tiles, the halo and the strip --------------------------------------------------------------

@pytest.mark.parametrize("H,W,T,size,radii", [(33, 65, 300, (3.0, 25.0), (1, 8)), (5, 3, 12, (1.0, 6.0), (8,))])
def test_frames_that_do_not_fit_the_tiles(oracle, H, W, T, size, radii):
    """One pixel past a tile both ways; and a frame smaller than the halo."""
    s = _Scene(oracle, random_soup(np.random.default_rng(H), T, max(H, W), size_px=size), H, W)
    assert s.covered > 3
    f = filler(H, W)
    for radius_px in radii:
        for fill in (None, FILL):
            s.check(f, f"{H} x {W}, radius {radius_px}, fill {fill}", color=LINE, fill=fill, radius_px=radius_px, width=3.0)


def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_alone(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    for fill in (None, FILL):
        for radius_px in (3, 8):
            s.draw(f)
            f.synchronize()
            # rows outside the strip: colours to be kept, and winners that WOULD draw if the pass looked at them
            f.color_buffer[:y0] = 7.5
            f.color_buffer[y1:] = -2.25
            f.winner_buffer[:y0] = 0
            f.winner_buffer[y1:] = 1
            f.wire_pass(width=3.0, color=LINE, fill=fill, outline=True, radius_px=radius_px)
            got = host(f.get_color_tensor())
            assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
            want = s.want(width=3.0, color=LINE, fill=fill, radius_px=radius_px, y0=y0, y1=y1)
            assert (want[y0:y1].view(np.uint32) != s.cam.color_buffer[y0:y1].view(np.uint32)).any()
            assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, fill {fill}, radius {radius_px}")


# ---- 3. random soups -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,T,H,W,size,presort", [
    (51, 4000, 200, 173, (1.0, 40.0), None),
    (73, 3000, 512, 509, (3.0, 60.0), True),
])
def test_random_soups(oracle, seed, T, H, W, size, presort):
    s = _Scene(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), size_px=size), H, W)
    f = filler(H, W, presort=presort)
    # the mask is indexed in the caller's order while the corners are fetched through d_pos_of: a random mask tells
    # a mix-up of the two orders
    mask = edge_mask("random", s.tri, seed)
    s.check(f, f"soup{seed}", color=LINE)
    s.check(f, f"soup{seed}, masked", mask_key="random", color=LINE, edges=mask, width=2.0)
    s.check(f, f"soup{seed}, masked and filled", mask_key="random", color=LINE, edges=mask, fill=FILL, width=2.0, feather=0.5)
    if presort:
        assert f._order is not None        # the resident inputs are the tile-coherent copies: the pass went through d_pos_of
        perm = np.random.default_rng(1).permutation(T)
        assert (s.want(edges=mask[perm], width=2.0) != s.want(mask_key="random", edges=mask, width=2.0)).any()


# ---- 4. special values, through the C entry ------------------------------------------------------------------------

def _outline(lib, winner, z, tri, P, color, width=1.0, feather=1.0, opacity=1.0, line=LINE, fill=None, edges=None, T=None,
             pos_of=None, depth_bias=1e-3, radius_px=2):
    import torch
    from cython3dmodelrenderer_amd import _capi
    T = tri.shape[0] if T is None else T
    H, W = winner.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.crender_wire_outline(
        winner.data_ptr(), z.data_ptr(), tri.data_ptr() if T else None, T, None if pos_of is None else pos_of.data_ptr(),
        _capi.f32_16(P), None if edges is None else edges.data_ptr(), (C.c_float * 3)(*line),
        None if fill is None else (C.c_float * 3)(*fill), width, feather, opacity, depth_bias, radius_px, color.data_ptr(),
        H, W, 0, H, 0, st), "crender_wire_outline")
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
    # corners that are NaN, infinite, huge or zero; triangles with two equal corners (an edge of no length); winners
    # that name no triangle, or a triangle far from the pixel; a z plane with NaN and infinities
    odd = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0])
    tri = tri.copy()
    hit = rng.uniform(size=tri.shape) < 0.05
    tri[hit] = rng.choice(odd, int(hit.sum()))
    twice = rng.uniform(size=T) < 0.1
    tri[twice, 1] = tri[twice, 0]
    bad = np.int32([-1, -2, T, T + 1, 2 ** 31 - 1, -2 ** 31])
    winner = cam.winner.copy()
    hit = rng.uniform(size=winner.shape) < 0.1
    winner[hit] = rng.choice(bad, int(hit.sum()))
    hit = rng.uniform(size=winner.shape) < 0.1
    winner[hit] = rng.integers(0, T, int(hit.sum()))
    z = cam.z_buffer.copy()
    hit = rng.uniform(size=z.shape) < 0.1
    z[hit] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 0.0]), int(hit.sum()))
    color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    mask = rng.integers(0, 8, T).astype(np.uint8)
    named = (winner >= 0) & (winner < T)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(winner=winner, tri=tri, mask=mask, z=z).items()}

    def model(w=winner, **kw):
        kw = dict(kw)
        e = kw.pop("edges", None)
        counts = {}
        out = outline_ref.wire_pass(color, w, z, tri, cam.proj_mat, edges=None if e is None else mask, counts=counts, **kw)
        assert not np.isnan(out).any()                   # a NaN distance is never taken: none reaches the colours
        return out, counts
    touched = nans = outside = 0
    for kw in (dict(), dict(width=3.0, feather=0.5, radius_px=3), dict(width=3.0, fill=FILL, depth_bias=0.0, radius_px=8),
               dict(edges=True, width=2.0, depth_bias=-2e-3), dict(edges=True, fill=FILL, width=0.5, feather=0.25, opacity=0.5),
               dict(width=64.0, feather=64.0, fill=FILL, radius_px=8), dict(width=2.0, radius_px=0, depth_bias=0.0)):
        kw.setdefault("radius_px", 2)
        want, counts = model(line=LINE, **kw)
        ckw = dict(kw)
        if ckw.pop("edges", None):
            ckw["edges"] = dev["mask"]
        got = _outline(lib, dev["winner"], dev["z"], dev["tri"], cam.proj_mat, torch.from_numpy(color).cuda(), **ckw)
        assert_bit_equal(got, want, f"odd values, {kw}")
        assert not np.isnan(got).any()
        if "fill" in kw:
            assert (got[named] != color[named]).any(1).all()         # every covered pixel is stored
        touched = max(touched, int((want.view(np.uint32) != color.view(np.uint32)).any(2).sum()))
        outside = max(outside, counts["background_on"])
        nans = max(nans, counts["nan"])
    assert touched > 500 and nans > 50 and outside > 20
    for name in ("winner", "z", "tri"):
        assert_bit_equal(host(dev[name]), dict(winner=winner, z=z, tri=tri)[name], f"{name} is only read")
    # an entry of d_pos_of beyond T makes its triangle background, as a pixel's own winner and as a neighbour's; the
    # others are found where it says, their edge bits where the caller put them
    perm = rng.permutation(T).astype(np.uint32)
    moved = np.empty_like(tri)
    moved[perm] = tri
    pos_of = perm.copy()
    gone = rng.uniform(size=T) < 0.3
    pos_of[gone] = rng.choice(np.uint32([T, T + 7, 2 ** 32 - 1]), int(gone.sum()))
    visible = np.where(winner >= 0, winner, 0)
    masked = np.where(named & gone[np.clip(visible, 0, T - 1)], -1, winner).astype(np.int32)
    for kw in (dict(width=3.0, edges=True, radius_px=3), dict(width=3.0, edges=True, fill=FILL, radius_px=3)):
        ckw = dict(kw, edges=dev["mask"])
        got = _outline(lib, dev["winner"], dev["z"], torch.from_numpy(moved).cuda(), cam.proj_mat, torch.from_numpy(color).cuda(),
                       pos_of=torch.from_numpy(pos_of.view(np.int32)).cuda(), **ckw)
        assert_bit_equal(got, model(masked, line=LINE, **kw)[0], f"d_pos_of with entries beyond T, {kw}")
    # no triangles, and a frame that is background only: nothing is written
    for kw in (dict(T=0), dict()):
        w = dev["winner"] if kw else torch.full((H, W), -1, dtype=torch.int32).cuda()
        for fill in (None, FILL):
            got = _outline(lib, w, dev["z"], dev["tri"], cam.proj_mat, torch.from_numpy(color).cuda(), fill=fill, radius_px=8, **kw)
            assert_bit_equal(got, color, f"nothing to draw, {kw}, fill {fill}")


# ---- 5. inputs and host views --------------------------------------------------------------------------------------

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
    kw = dict(width=2.0, color=LINE, fill=FILL)
    want = s.want(mask_key="all", **kw)
    assert (want != s.cam.color_buffer).any()
    f = filler(256, 256)                          # numpy
    s.draw(f)
    f.wire_pass(outline=True, **kw)
    assert_bit_equal(host(f.get_color_tensor()), want, "numpy inputs")
    f = filler(256, 256)                          # caller's device tensors
    f.render_arrays(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tri, col, nrm)], clear=True)
    f.wire_pass(outline=True, **kw)
    assert_bit_equal(host(f.get_color_tensor()), want, "torch inputs")
    f = filler(256, 256)                          # the device-resident model
    f.render_model(DeviceModel(m), clear=True)
    f.wire_pass(outline=True, **kw)
    assert_bit_equal(host(f.get_color_tensor()), want, "DeviceModel inputs")
    s.check_planes(f, "DeviceModel inputs")


def test_host_views_show_the_lines_at_the_next_getter_call(soup256):
    s = soup256
    f = filler(256, 256)
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    f.wire_pass(width=2.0, color=LINE, outline=True)
    again = f.get_color_buffer()
    assert again is view
    assert_bit_equal(view, s.want(mask_key="all", width=2.0, color=LINE), "after the pass")
    # an edit of the colour's host view is what the lines are blended over
    s.draw(f)
    c = f.get_color_buffer()
    c[:] = np.float32([10.0, 100.0, 200.0])
    f.wire_pass(width=2.0, color=LINE, opacity=0.5, outline=True)
    flat = np.broadcast_to(np.float32([10.0, 100.0, 200.0]), s.cam.color_buffer.shape)
    edited = s.want(base=flat, mask_key="all", width=2.0, color=LINE, opacity=0.5)
    assert (edited != s.want(mask_key="all", color=LINE, width=2.0, opacity=0.5)).any()
    assert_bit_equal(f.get_color_buffer(), edited, "over edited colours")


# ---- 6. Renderer ---------------------------------------------------------------------------------------------------

WIRE = dict(width=2.0, color=LINE, feather=0.5, outline=True, depth_bias=2e-3, radius_px=3)
SOUP_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.25)]
PHONG_KW = dict(ambient=0.15, shininess=16)


def test_renderer_with_supersampling(soup256):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    ill = GuroIllumination(GURO)
    f = filler(256, 256)
    out = Renderer(f, ill, None, 128, 128, on_device=True, wireframe=WIRE, supersample=2).render(s.model)
    got = host(out)
    assert got.shape == (128, 128, 3)
    a = filler(256, 256)
    a.render_model(s.model, clear=True)
    ill.draw_illumination_device(a)
    lit = host(a.get_color_tensor()).copy()
    a.wire_pass(**WIRE)
    assert_bit_equal(host(f.get_color_tensor()), s.want(base=lit, mask_key="all", **WIRE), "the supersampled frame is the model's")
    assert_bit_equal(got, host(a.resolve(2)), "the illumination pass, wire_pass, resolve(2)")
    b = filler(256, 256)
    b.render_model(s.model, clear=True)
    ill.draw_illumination_device(b)
    b.wire_pass(**dict(WIRE, outline=False))
    assert (got != host(b.resolve(2))).any()      # the options reached the pass
    s.check_planes(f, "after the supersampled frame")


def test_renderer_draws_the_outline_after_the_shadow(oracle, soup256):
    from cython3dmodelrenderer_amd import shadow
    from cython3dmodelrenderer_amd.illumination import PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    R, t = shadow_ref.rotation_frame(s.tri, (10, -20, 0))
    ltri, lnrm = shadow.light_arrays(s.tri, s.nrm, R, t)
    lig = oracle.OracleFiller(128, 160, fov=45.0)
    lig.render_arrays(ltri, s.col, lnrm)

    def shadowed(color):
        return shadow_ref.shadow_pass(color, s.cam.winner, s.tri, s.cam.proj_mat, ltri, lig.proj_mat, lig.z_buffer,
                                      lig.winner, bias=2e-3, ambient=0.125, pcf=3)
    lit = phong_ref.phong_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.cam.normals_buffer, SOUP_LIGHTS,
                               **PHONG_KW)
    want = s.want(base=shadowed(lit), mask_key="all", **WIRE)
    other = shadowed(s.want(base=lit, mask_key="all", **WIRE))
    assert (want != other).any()                   # lines inside a shadow: the two orders differ on this scene
    f, g = filler(256, 256), filler(128, 160)
    r = Renderer(f, PhongIllumination(lights=SOUP_LIGHTS, **PHONG_KW), on_device=True,
                 shadow=dict(filler=g, R=R, t=t, bias=2e-3, pcf=3, ambient=0.125), wireframe=WIRE)
    got = host(r.render(s.model))
    assert_bit_equal(got, want, "Renderer(PhongIllumination, shadow=..., wireframe={outline...})")
    a, b = filler(256, 256), filler(128, 160)    # and by hand
    s.draw(a)
    b.render_arrays(ltri, s.col, lnrm, clear=True)
    a.bind_shadow_map(b, ltri)
    a.phong_pass(SOUP_LIGHTS, **PHONG_KW)
    a.shadow_pass(bias=2e-3, pcf=3, ambient=0.125)
    a.wire_pass(**WIRE)
    assert_bit_equal(got, host(a.get_color_tensor()), "phong_pass, shadow_pass, wire_pass")


def test_renderer_with_a_texture_pass(soup256):
    from cython3dmodelrenderer_amd.data_structures.model import Model
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    rng = np.random.default_rng(72)
    T = len(s.tri)
    idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    uv = rng.uniform(0, 1, (T, 3, 2)).astype(np.float32)
    tex = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    m = Model(s.tri.reshape(-1, 3), idx, uv.reshape(-1, 2), idx, tex, s.nrm.reshape(-1, 3), idx, recalculate_normals=False)
    f = filler(256, 256)
    got = host(Renderer(f, GuroIllumination(GURO), on_device="fused", texture_pass={"perspective": True},
                         wireframe=WIRE).render(m))
    a = filler(256, 256)
    a.bind_texture(m.get_texture_coords_by_triangles(), tex)
    a.render_model(m, clear=True)
    a.texture_pass(perspective=True, light_direction=GuroIllumination(GURO).light_direction)
    textured = host(a.get_color_tensor()).copy()
    assert (textured != s.cam.color_buffer).any()
    assert_bit_equal(got, s.want(base=textured, mask_key="all", **WIRE), "the texture with its light, then the outline")
    a.wire_pass(**WIRE)
    assert_bit_equal(got, host(a.get_color_tensor()), "texture_pass, wire_pass")


# ---- 7. errors -----------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(soup256):
    s = soup256
    f = filler(256, 256, track_winner=False)
    s.draw(f)
    with pytest.raises(ValueError, match="winner plane"):
        f.wire_pass(outline=True)
    f = filler(256, 256)
    with pytest.raises(ValueError, match="no frame has been rendered"):
        f.wire_pass(outline=True)
    s.draw(f)
    f.render_arrays(s.tri, s.col, s.nrm)           # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.wire_pass(outline=True)
    with pytest.raises(ValueError, match="swap chain"):
        filler(64, 64, pipeline=True).wire_pass(outline=True)
    s.draw(f)
    T = len(s.tri)
    for kw, word in ((dict(radius_px=-1), "radius_px must be"), (dict(radius_px=9), "radius_px must be"),
                     (dict(radius_px=2.0), "radius_px must be"), (dict(radius_px=True), "radius_px must be"),
                     (dict(depth_bias=float("nan")), "depth_bias must be"), (dict(depth_bias=float("inf")), "depth_bias must be"),
                     (dict(depth_bias="0"), "depth_bias must be"), (dict(width=10.0, feather=4.5), "at most 14"),
                     (dict(width=0.0), "width must be"), (dict(opacity=2), "opacity must be")):
        with pytest.raises(ValueError, match=word):
            f.wire_pass(outline=True, **kw)
    with pytest.raises(ValueError, match=rf"T = {T}.*\({T - 1},\)"):
        f.wire_pass(outline=True, edges=np.zeros(T - 1, np.uint8))
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "nothing was written")
    f.wire_pass(outline=True, width=10.0, feather=4.0)                 # the widest line that fits: radius 8
    assert_bit_equal(host(f.get_color_tensor()), s.want(width=10.0, feather=4.0), "the widest line")
    s.draw(f)
    f.wire_pass(**WIRE)                            # and works again
    assert_bit_equal(host(f.get_color_tensor()), s.want(mask_key="all", **WIRE), "after the errors")


# ---- 8. bin overflow -----------------------------------------------------------------------------------------------

def test_a_frame_redrawn_after_a_bin_overflow_ends_outlined(oracle):
    """The scene of test_a_frame_redrawn_after_a_bin_overflow_ends_lit: the bin lists are far too small, the frame
    drops fragments and is rendered again when it is settled — which the pass does before it launches."""
    s = _Scene(oracle, random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0), 512, 512)
    want = s.want(width=3.0, color=LINE)
    for kw in (dict(), dict(presort=True)):
        f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False, **kw)
        s.draw(f)
        need, cap = f.bin_usage()
        assert cap == 500 and need > cap and len(f._pending) == 1     # dropped fragments, nobody has looked yet
        f.wire_pass(width=3.0, color=LINE, outline=True)
        assert not f._pending                                          # grown and redone before the pass
        assert_bit_equal(host(f.get_color_tensor()), want, f"a redone frame, {kw}")
        s.check_planes(f, "a redone frame")
