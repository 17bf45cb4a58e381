"""The hidden-line overlay on the GPU (csrc/wireframe.hip's k_wire_overlay through AdvancedPixelBufferFiller.wire_pass
and Renderer(wireframe=...)), bit for bit against the host model of tests/overlay_ref.py evaluated on the oracle's
frames (itself pinned in tests/test_wire_pass_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import overlay_ref
import phong_ref
import shadow_ref
from pass_scenes import Scene, Soup, edge_mask, filler, host, soup_fixture, trex_arrays, trex_fixture
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)              # what GuroIllumination is constructed with
LINE = (250.0, 240.0, 20.0)
FILL = (30.0, 35.0, 40.0)
# (width, feather, opacity): thin, wide with a narrow ramp, and hair lines at half strength
STYLES = [dict(width=1.0, feather=1.0), dict(width=3.0, feather=0.5), dict(width=0.5, feather=0.25, opacity=0.5)]


class _Scene(Scene):
    def want(self, base=None, **kw):
        """The model's frame after ``wire_pass(**kw)`` over `base` (the oracle's colours if None)."""
        kw = dict(kw)
        kw["line"] = kw.pop("color", (255, 255, 255))
        return overlay_ref.wire_pass(self.cam.color_buffer if base is None else base, self.cam.winner, self.tri,
                                     self.cam.proj_mat, **kw)

    def check(self, f, what, **kw):
        self.draw(f)
        f.wire_pass(**kw)
        want = self.want(**kw)
        self.assert_changed(want, what)
        assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour")
        self.check_planes(f, what)
        return want


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


# ---- 1. T-Rex ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edges", ["all", "feature", "random"])
@pytest.mark.parametrize("fill", [None, FILL])
def test_trex_every_instance(trex256, fill, edges):
    import torch
    s = trex256
    assert s.covered == 15801
    f = filler(256, 256)
    mask = edge_mask(edges, s.tri)
    for style in STYLES:
        s.check(f, f"trex256, fill {fill}, {edges} edges, {style}", color=LINE, fill=fill, edges=mask, **style)
    if mask is not None:            # a device tensor is taken as it is
        s.draw(f)
        f.wire_pass(color=LINE, fill=fill, edges=torch.from_numpy(mask).cuda(), **STYLES[1])
        assert_bit_equal(host(f.get_color_tensor()), s.want(color=LINE, fill=fill, edges=mask, **STYLES[1]), "a device mask")


# ---- 2. random soups -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,T,H,W,size,presort", [
    (51, 4000, 200, 173, (1.0, 40.0), None),
    (71, 3000, 256, 256, (3.0, 50.0), None),
    (71, 3000, 256, 256, (3.0, 50.0), True),
])
def test_random_soups(oracle, seed, T, H, W, size, presort):
    s = _Scene(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), size_px=size), H, W)
    f = filler(H, W, presort=presort)
    # the mask is indexed in the caller's order while the corners are fetched through d_pos_of: a random mask tells
    # a mix-up of the two orders
    mask = edge_mask("random", s.tri, seed)
    for style in STYLES[:2]:
        s.check(f, f"soup{seed}", color=LINE, **style)
        s.check(f, f"soup{seed}, masked", color=LINE, edges=mask, **style)
        s.check(f, f"soup{seed}, masked and filled", color=LINE, edges=mask, fill=FILL, **style)
    if presort:
        assert f._order is not None        # the resident inputs are the tile-coherent copies: the pass went through d_pos_of
        perm = np.random.default_rng(1).permutation(T)
        assert (s.want(edges=mask[perm], width=3.0) != s.want(edges=mask, width=3.0)).any()      # the order matters here


def test_a_row_strip_of_an_odd_frame_leaves_the_other_rows_alone(oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    for fill in (None, FILL):
        s.draw(f)
        f.synchronize()
        # rows outside the strip: colours to be kept, and winners that WOULD draw if the pass looked at them
        f.color_buffer[:y0] = 7.5
        f.color_buffer[y1:] = -2.25
        f.winner_buffer[:y0] = 0
        f.winner_buffer[y1:] = 1
        f.wire_pass(width=3.0, color=LINE, fill=fill)
        got = host(f.get_color_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        want = s.want(width=3.0, color=LINE, fill=fill, y0=y0, y1=y1)
        assert (want[y0:y1].view(np.uint32) != s.cam.color_buffer[y0:y1].view(np.uint32)).any()
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, fill {fill}")


# ---- 3. special values and the window's decisions, through the C entry ---------------------------------------------

def _overlay(lib, winner, tri, P, color, width=1.0, feather=1.0, opacity=1.0, line=LINE, fill=None, edges=None, T=None,
             pos_of=None):
    import torch
    from cython3dmodelrenderer_amd import _capi
    T = tri.shape[0] if T is None else T
    H, W = winner.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.crender_wire_overlay(
        winner.data_ptr(), tri.data_ptr() if T else None, T, None if pos_of is None else pos_of.data_ptr(), _capi.f32_16(P),
        None if edges is None else edges.data_ptr(), (C.c_float * 3)(*line), None if fill is None else (C.c_float * 3)(*fill),
        width, feather, opacity, color.data_ptr(), H, W, 0, H, 0, st), "crender_wire_overlay")
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
    # corners that are NaN, infinite, huge or zero; triangles with two equal corners; winners that name no triangle
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
    color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    mask = rng.integers(0, 8, T).astype(np.uint8)
    named = (winner >= 0) & (winner < T)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(winner=winner, tri=tri, mask=mask).items()}

    def model(w=winner, **kw):
        kw = dict(kw)
        e = kw.pop("edges", None)
        counts = {}
        out = overlay_ref.wire_pass(color, w, tri, cam.proj_mat, edges=None if e is None else mask, counts=counts, **kw)
        assert not np.isnan(out).any()                   # a NaN distance is never taken: none reaches the colours
        return out, counts
    touched = nans = 0
    for kw in (dict(), dict(width=3.0, feather=0.5), dict(width=3.0, fill=FILL), dict(edges=True, width=2.0),
               dict(edges=True, fill=FILL, width=0.5, feather=0.25, opacity=0.5), dict(width=64.0, feather=64.0, fill=FILL)):
        want, counts = model(line=LINE, **kw)
        ckw = dict(kw)
        if ckw.pop("edges", None):
            ckw["edges"] = dev["mask"]
        got = _overlay(lib, dev["winner"], dev["tri"], cam.proj_mat, torch.from_numpy(color).cuda(), **ckw)
        assert_bit_equal(got, want, f"odd values, {kw}")
        assert_bit_equal(got[~named], color[~named], "what names no triangle is not written")
        if "fill" in kw:
            assert not np.isnan(got).any()
            assert (got[named] != color[named]).any(1).all()         # every covered pixel is stored
        touched = max(touched, int((want.view(np.uint32) != color.view(np.uint32)).any(2).sum()))
        nans = max(nans, counts["nan"])
    assert touched > 500 and nans > 50
    # an entry of d_pos_of beyond T makes its triangle background; the others are found where it says, their edge
    # bits where the caller put them
    perm = rng.permutation(T).astype(np.uint32)
    moved = np.empty_like(tri)
    moved[perm] = tri
    pos_of = perm.copy()
    gone = rng.uniform(size=T) < 0.3
    pos_of[gone] = rng.choice(np.uint32([T, T + 7, 2 ** 32 - 1]), int(gone.sum()))
    visible = np.where(winner >= 0, winner, 0)
    masked = np.where(named & gone[np.clip(visible, 0, T - 1)], -1, winner).astype(np.int32)
    for kw in (dict(width=3.0, edges=True), dict(width=3.0, edges=True, fill=FILL)):
        ckw = dict(kw, edges=dev["mask"])
        got = _overlay(lib, dev["winner"], torch.from_numpy(moved).cuda(), cam.proj_mat, torch.from_numpy(color).cuda(),
                       pos_of=torch.from_numpy(pos_of.view(np.int32)).cuda(), **ckw)
        assert_bit_equal(got, model(masked, line=LINE, **kw)[0], f"d_pos_of with entries beyond T, {kw}")
    # no triangles, and a frame that is background only: nothing is written
    for kw in (dict(T=0), dict()):
        w = dev["winner"] if kw else torch.full((H, W), -1, dtype=torch.int32).cuda()
        for fill in (None, FILL):
            got = _overlay(lib, w, dev["tri"], cam.proj_mat, torch.from_numpy(color).cuda(), fill=fill, **kw)
            assert_bit_equal(got, color, f"nothing to draw, {kw}, fill {fill}")


def test_the_windows_two_decisions_taken_both_ways():
    """With ones on the diagonal, z = 1 and W = H = 32 a vertex lands on x' = (x + 1) * 16 exactly.  Triangle 0 has its
    edge 0 on the column x' = 8, triangle 1 on x' = 8.5, both 16 rows long (a power of two: the distances are exact).
    At width 3, feather 1 a pixel at distance d has a = 2 - d: at exactly 2 it is NOT written, at exactly 1 it has all
    of the line, at 1.5 half of it."""
    import torch
    from cython3dmodelrenderer_amd import _capi
    lib = _capi.load()
    H = W = 32
    P = np.eye(4, dtype=np.float32)
    tri = np.float32([[[-0.5, -0.5, 1.0], [-0.5, 0.5, 1.0], [0.5, 0.0, 1.0]],
                      [[-0.46875, -0.5, 1.0], [-0.46875, 0.5, 1.0], [0.5, 0.0, 1.0]]])
    winner = np.zeros((H, W), np.int32)
    winner[16:] = 1                                   # (the pass asks the winner plane, not the triangle, who is inside)
    winner[:, 20:] = -1
    rng = np.random.default_rng(2)
    color = rng.uniform(1, 200, (H, W, 3)).astype(np.float32)
    edges = np.uint8([1, 1])
    line = (255.0, 255.0, 255.0)
    got = _overlay(lib, torch.from_numpy(winner).cuda(), torch.from_numpy(tri).cuda(), P, torch.from_numpy(color).cuda(),
                   width=3.0, feather=1.0, line=line, edges=torch.from_numpy(edges).cuda())
    want = overlay_ref.wire_pass(color, winner, tri, P, width=3.0, feather=1.0, line=line, edges=edges)
    assert_bit_equal(got, want, "the two columns")
    top, low = got[:16], got[16:]
    for x in (7, 8, 9):                               # distance 1, 0, 1: a = 1
        assert (top[:, x] == 255.0).all(), x
    for x in (6, 10):                                 # distance exactly 2: a = 0 is not "on", the pixel keeps its bits
        assert_bit_equal(top[:, x], color[:16, x], f"column {x}")
    assert_bit_equal(top[:, :6], color[:16, :6], "left of the line")
    assert_bit_equal(top[:, 11:], color[:16, 11:], "right of the line")
    for x in (8, 9):                                  # distance 0.5: a = 1.5 -> 1
        assert (low[:, x] == 255.0).all(), x
    for x in (7, 10):                                 # distance 1.5: a = 0.5
        assert_bit_equal(low[:, x], color[16:, x] * np.float32(0.5) + np.float32(127.5), f"column {x}")
    for x in (6, 11):                                 # distance 2.5
        assert_bit_equal(low[:, x], color[16:, x], f"column {x}")
    # with a fill the pixel at distance exactly 2 holds the fill, not a blend
    got = _overlay(lib, torch.from_numpy(winner).cuda(), torch.from_numpy(tri).cuda(), P, torch.from_numpy(color).cuda(),
                   width=3.0, feather=1.0, line=line, fill=FILL, edges=torch.from_numpy(edges).cuda())
    assert (got[:16, 10] == np.float32(FILL)).all() and (got[:16, 9] == 255.0).all()
    assert_bit_equal(got[16:, 10], np.broadcast_to(np.float32(FILL) * np.float32(0.5) + np.float32(127.5), (16, 3)), "half")
    assert_bit_equal(got[:, 20:], color[:, 20:], "the background")


# ---- 4. host views -------------------------------------------------------------------------------------------------

def test_host_views_show_the_lines_at_the_next_getter_call(soup256):
    s = soup256
    f = filler(256, 256)
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    f.wire_pass(width=2.0, color=LINE)
    again = f.get_color_buffer()
    assert again is view
    assert_bit_equal(view, s.want(width=2.0, color=LINE), "after the pass")
    # an edit of the colour's host view is what the lines are blended over
    s.draw(f)
    c = f.get_color_buffer()
    c[:] = np.float32([10.0, 100.0, 200.0])
    f.wire_pass(width=2.0, color=LINE, opacity=0.5)
    flat = np.broadcast_to(np.float32([10.0, 100.0, 200.0]), s.cam.color_buffer.shape)
    want = s.want(color=LINE, width=2.0, opacity=0.5)
    edited = overlay_ref.wire_pass(flat, s.cam.winner, s.tri, s.cam.proj_mat, width=2.0, line=LINE, opacity=0.5)
    assert (edited != want).any()
    assert_bit_equal(f.get_color_buffer(), edited, "over edited colours")


# ---- 5. Renderer ---------------------------------------------------------------------------------------------------

WIRE = dict(width=2.0, color=LINE, feather=0.5)


def _by_hand(s, on_device, **wire):
    """draw, the illumination in the form `on_device` names, then the wire pass."""
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    a = filler(256, 256)
    ill = GuroIllumination(GURO)
    if on_device == "fused":
        ill.fuse_into(a)
    a.render_model(s.model, clear=True)
    if on_device is False:
        ill.draw_illumination(a.get_color_buffer(), a.get_normals_buffer())
    elif on_device != "fused":
        ill.draw_illumination_device(a)
    lit = host(a.get_color_tensor()).copy() if on_device is not False else None
    a.wire_pass(**wire)
    return host(a.get_color_tensor()), lit


@pytest.mark.parametrize("on_device", [None, True, False, "fused"])
def test_renderer_draws_the_lines_over_the_light(soup256, on_device):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    want, lit = _by_hand(s, on_device, **WIRE)
    if lit is not None:                            # and the hand composition is the model's: unlit lines over the lit frame
        assert_bit_equal(want, s.want(base=lit, **WIRE), "the hand composition")
        assert (want != lit).any()
    f = filler(256, 256)
    r = Renderer(f, GuroIllumination(GURO), on_device=on_device, wireframe=WIRE)
    for _ in range(2):                             # every frame starts from cleared buffers
        out = r.render(s.model)
        assert isinstance(out, np.ndarray) == (on_device in (None, False))
        assert_bit_equal(np.array(out) if isinstance(out, np.ndarray) else host(out), want, f"Renderer(on_device={on_device!r})")
    s.check_planes(f, "after Renderer")


def test_renderer_feature_angle_is_the_feature_mask(soup256, trex256):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    tri = trex256.tri
    m = Soup.__new__(Soup)
    m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles = tri, trex256.col, trex256.nrm
    f = filler(256, 256)
    r = Renderer(f, GuroIllumination(GURO), on_device=True, wireframe=dict(WIRE, feature_angle=30))
    got = host(r.render(m))
    kept = r._wired[1]
    assert_bit_equal(host(r.render(m)), got, "the second frame")
    assert r._wired[1] is kept                     # once per model
    a = filler(256, 256)
    a.render_model(m, clear=True)
    GuroIllumination(GURO).draw_illumination_device(a)
    lit = host(a.get_color_tensor()).copy()
    a.wire_pass(edges=feature_edges(tri, 30.0), **WIRE)
    assert_bit_equal(got, host(a.get_color_tensor()), "feature_angle=30")
    assert_bit_equal(got, trex256.want(base=lit, edges=feature_edges(tri, 30.0), **WIRE), "the model")
    assert (got != trex256.want(base=lit, **WIRE)).any()
    # another model: another mask
    s = soup256
    got = host(r.render(s.model))
    assert len(r._wired[1]) == len(s.tri)
    assert_bit_equal(got, _by_hand(s, True, edges=feature_edges(s.tri, 30.0), **WIRE)[0], "the next model")


SOUP_LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.5), dict(direction=(0.5, 0.3, 1.0), diffuse=0.3, specular=0.25)]
PHONG_KW = dict(ambient=0.15, shininess=16)


def test_renderer_draws_the_lines_after_the_shadow(oracle, soup256):
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
    want = s.want(base=shadowed(lit), **WIRE)
    other = shadowed(s.want(base=lit, **WIRE))
    assert (want != other).any()                   # lines inside a shadow: the two orders differ on this scene
    f, g = filler(256, 256), filler(128, 160)
    r = Renderer(f, PhongIllumination(lights=SOUP_LIGHTS, **PHONG_KW), on_device=True,
                 shadow=dict(filler=g, R=R, t=t, bias=2e-3, pcf=3, ambient=0.125), wireframe=WIRE)
    assert_bit_equal(host(r.render(s.model)), want, "Renderer(PhongIllumination, shadow=..., wireframe=...)")


@pytest.mark.parametrize("on_device", [None, True])
def test_renderer_with_supersampling(soup256, on_device):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    ill = GuroIllumination(GURO)
    out = Renderer(filler(256, 256), ill, None, 128, 128, on_device=on_device, wireframe=WIRE, supersample=2).render(s.model)
    assert isinstance(out, np.ndarray) == (on_device is None)
    got = out if on_device is None else host(out)
    assert got.shape == (128, 128, 3)
    a = filler(256, 256)
    a.render_model(s.model, clear=True)
    ill.draw_illumination_device(a)
    a.wire_pass(**WIRE)
    assert_bit_equal(got, host(a.resolve(2)), "the illumination pass, wire_pass, resolve(2)")
    # the light in the resolve would shade the lines
    b = filler(256, 256)
    b.render_model(s.model, clear=True)
    b.wire_pass(**WIRE)
    assert (got != host(b.resolve(2, light_direction=ill.light_direction))).any()


# ---- 6. errors -----------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(soup256):
    s = soup256
    f = filler(256, 256, track_winner=False)
    s.draw(f)
    with pytest.raises(ValueError, match="winner plane"):
        f.wire_pass()
    f = filler(256, 256)
    with pytest.raises(ValueError, match="no frame has been rendered"):
        f.wire_pass()
    s.draw(f)
    f.render_arrays(s.tri, s.col, s.nrm)           # composites on the frame before
    with pytest.raises(ValueError, match="did not start from cleared buffers"):
        f.wire_pass()
    with pytest.raises(ValueError, match="swap chain"):
        filler(64, 64, pipeline=True).wire_pass()
    s.draw(f)
    T = len(s.tri)
    for kw, word in ((dict(width=0.0), "width"), (dict(width=65), "width"), (dict(width=float("nan")), "width"),
                     (dict(feather=0), "feather"), (dict(feather=100.0), "feather"), (dict(feather=float("inf")), "feather"),
                     (dict(opacity=-0.5), "opacity"), (dict(opacity=2), "opacity"), (dict(opacity=float("nan")), "opacity")):
        with pytest.raises(ValueError, match=word + " must be"):
            f.wire_pass(**kw)
    with pytest.raises(ValueError, match=rf"T = {T}.*\({T - 1},\)"):
        f.wire_pass(edges=np.zeros(T - 1, np.uint8))
    with pytest.raises(ValueError, match=rf"T = {T}.*int32"):
        f.wire_pass(edges=np.zeros(T, np.int32))
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "nothing was written")
    f.wire_pass(**WIRE)                            # and works again
    assert_bit_equal(host(f.get_color_tensor()), s.want(**WIRE), "after the errors")


# ---- 7. bin overflow -----------------------------------------------------------------------------------------------

def test_a_frame_redrawn_after_a_bin_overflow_ends_wired(oracle):
    """The scene of test_a_frame_redrawn_after_a_bin_overflow_ends_lit: the bin lists are far too small, the frame
    drops fragments and is rendered again when it is settled — which the pass does before it launches."""
    s = _Scene(oracle, random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0), 512, 512)
    want = s.want(width=3.0, color=LINE)
    for kw in (dict(), dict(presort=True)):
        f = filler(512, 512, tile=32, bin_capacity=500, direct_bins=False, **kw)
        s.draw(f)
        need, cap = f.bin_usage()
        assert cap == 500 and need > cap and len(f._pending) == 1     # dropped fragments, nobody has looked yet
        f.wire_pass(width=3.0, color=LINE)
        assert not f._pending                                          # grown and redone before the pass
        assert_bit_equal(host(f.get_color_tensor()), want, f"a redone frame, {kw}")
        s.check_planes(f, "a redone frame")
