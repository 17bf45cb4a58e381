"""The deferred shadow pass on the GPU (csrc/shadow.hip through AdvancedPixelBufferFiller.shadow_pass and
Renderer(shadow=...)), bit for bit against the host model of tests/shadow_ref.py evaluated on the oracle's frames
(itself pinned by hand and on T-Rex in tests/test_shadow_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import shadow_ref
from pass_scenes import GOLDEN, Scene, Soup, filler, host, planes_only_read, trex_arrays
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

EVERY = [(K, w) for K in (1, 3, 5) for w in (False, True)]
LIGHT = (0.3, -0.2, 1.0)             # what GuroIllumination is constructed with
BIAS, AMBIENT = 1e-3, 0.25


class _Scene(Scene):
    """A model, its light-frame arrays and the oracle's two frames of it: computed once, only read afterwards."""

    def __init__(self, oracle, arrays, H, W, Hl, Wl, R, t, light_fov=45.0, y0=0, y1=None):
        from cython3dmodelrenderer_amd import shadow
        super().__init__(oracle, arrays, H, W, y0, y1)
        self.Hl, self.Wl, self.light_fov = Hl, Wl, light_fov
        self.R, self.t = R, t
        self.ltri, self.lnrm = shadow.light_arrays(self.tri, self.nrm, R, t)
        self.lig = oracle.OracleFiller(Hl, Wl, fov=light_fov)
        self.lig.render_arrays(self.ltri, self.col, self.lnrm)

    def want(self, K=1, use_winner=True, bias=BIAS, ambient=AMBIENT, color=None, counts=None, **kw):
        return shadow_ref.shadow_pass(self.cam.color_buffer if color is None else color, self.cam.winner, self.tri,
                                      self.cam.proj_mat, self.ltri, self.lig.proj_mat, self.lig.z_buffer,
                                      self.lig.winner if use_winner else None, bias=bias, ambient=ambient, pcf=K,
                                      counts=counts, **kw)

    def fillers(self, camera_kw=None, light_kw=None):
        return filler(self.H, self.W, **(camera_kw or {})), filler(self.Hl, self.Wl, fov=self.light_fov, **(light_kw or {}))

    def draw(self, f, g):
        super().draw(f)
        g.render_arrays(self.ltri, self.col, self.lnrm, clear=True)
        f.bind_shadow_map(g, self.ltri)

    def check_planes(self, f, g, what):
        """z, normals and the winner planes of both fillers are only read."""
        planes_only_read(f, self.cam, f"{what}: the camera")
        planes_only_read(g, self.lig, f"{what}: the light")

    def off_the_map(self):
        """(share of the covered pixels whose texel is off the map, share whose surface point is behind the light)."""
        from oracle import oracle as O
        _, _, t, X, Y, Z = shadow_ref.light_point(self.cam.winner, self.tri, self.cam.proj_mat, self.ltri)
        with np.errstate(all="ignore"):
            p = O.project(np.ascontiguousarray(np.stack([X, Y, Z], 1)[:, None, :].repeat(3, 1)), self.lig.proj_mat,
                          self.Wl, self.Hl)[:, 0]
        behind = ~(Z > 0)
        off = ~behind & ~((p[:, 0] >= -0.5) & (p[:, 0] < self.Wl - 0.5) & (p[:, 1] >= -0.5) & (p[:, 1] < self.Hl - 0.5))
        return off.sum() / len(t), behind.sum() / len(t)

    def check(self, combos, what, f=None, g=None, changes=True, **pass_kw):
        if f is None:
            f, g = self.fillers()
        for K, use_winner in combos:
            self.draw(f, g)
            f.shadow_pass(bias=BIAS, pcf=K, ambient=AMBIENT, use_winner=use_winner, **pass_kw)
            want = self.want(K, use_winner)
            assert not np.isnan(want).any()
            assert_bit_equal(host(f.get_color_tensor()), want, f"{what} colour, K={K}, use_winner={use_winner}")
            if changes:
                self.assert_changed(want, what)
            self.check_planes(f, g, what)
        return f, g


@pytest.fixture(scope="module")
def trex256(oracle):
    """T-Rex at 256 x 256 with a 256 x 256 map, both fov 45; the light's frame holds the model turned about the
    float32 mean of its corners by the y block [[cos 40, -sin 40], [sin 40, cos 40]]: ``Model.rotate((0, -40, 0))`` in
    that method's own sign convention, the frame of the figures in tests/test_shadow_cpu.py."""
    arrays = trex_arrays()
    return _Scene(oracle, arrays, 256, 256, 256, 256, *shadow_ref.rotation_frame(arrays[0], (0, -40, 0)))


@pytest.fixture(scope="module")
def odd_trex(oracle):
    """T-Rex 200 x 173 under a 96 x 80 map of a light of fov 30 turned by (-25, 50, 0) in ``Model.rotate``'s convention
    (the blocks [[cos, -sin], [sin, cos]] of 25 and -50 degrees): most of the scene falls off the map."""
    arrays = trex_arrays()
    return _Scene(oracle, arrays, 200, 173, 96, 80, *shadow_ref.rotation_frame(arrays[0], (-25, 50, 0)), light_fov=30.0)


# ---- 1. T-Rex ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,use_winner", EVERY)
def test_trex_every_instance(trex256, K, use_winner):
    s = trex256
    assert s.covered == 15801
    s.check([(K, use_winner)], "trex256")
    if K == 1:
        counts = {}
        s.want(1, use_winner, counts=counts)
        # the host model on the oracle's frames: 88.1 % untouched, 11.9 % fully shadowed (with the rule 88.2 / 11.8)
        assert counts["shadowed"] >= 0.05 * s.covered and counts["lit"] >= 0.50 * s.covered
        assert counts["lit"] == (13934 if use_winner else 13923)


def test_trex_turned_the_other_way(oracle):
    """The same scene with the y block of ``Model.rotate((0, 40, 0))``: the light on the model's other side.
    The host model gives 67.6 % untouched, 32.4 % fully shadowed."""
    arrays = trex_arrays()
    s = _Scene(oracle, arrays, 256, 256, 256, 256, *shadow_ref.rotation_frame(arrays[0], (0, 40, 0)))
    s.check([(1, True)], "trex256, +40")
    counts = {}
    s.want(counts=counts)
    assert counts["shadowed"] >= 0.05 * s.covered and counts["lit"] >= 0.50 * s.covered


def test_without_a_bias_the_winner_rule_lights_strictly_more(trex256):
    s = trex256
    f, g = s.fillers()
    lit = {}
    for use_winner in (False, True):
        s.draw(f, g)
        f.shadow_pass(bias=0.0, pcf=1, ambient=AMBIENT, use_winner=use_winner)
        got = host(f.get_color_tensor())
        counts = {}
        assert_bit_equal(got, s.want(1, use_winner, bias=0.0, counts=counts), f"bias 0, use_winner={use_winner}")
        untouched = (got.view(np.uint32) == s.cam.color_buffer.view(np.uint32)).all(2) & (s.cam.winner >= 0)
        # (a black pixel stays black under any factor: the colour plane can only under-count the shadowed ones)
        assert int(untouched.sum()) >= counts["lit"]
        lit[use_winner] = counts["lit"]
    assert lit == {False: 7634, True: 12457} and lit[True] > lit[False]       # 48.3 % and 78.8 % of 15 801


# ---- 2. the light at the camera ------------------------------------------------------------------------------------

def test_the_light_at_the_camera_shadows_nothing(trex256):
    s = trex256
    f = filler(256, 256)
    f.render_arrays(s.tri, s.col, s.nrm, clear=True)
    f.bind_shadow_map(f, s.tri)          # R = I, t = 0, the same projection: the frame's own z and winner planes are the map
    f.shadow_pass(bias=0.0, pcf=1, use_winner=True)
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "bias 0 with the winner rule: 15 801 of 15 801 lit")

    def model(bias, lwinner):
        counts = {}
        want = shadow_ref.shadow_pass(s.cam.color_buffer, s.cam.winner, s.tri, s.cam.proj_mat, s.tri, s.cam.proj_mat,
                                      s.cam.z_buffer, lwinner, bias=bias, ambient=AMBIENT, counts=counts)
        return want, counts["lit"]
    # without the rule the depth a pixel carries into the map and the depth stored there are two roundings of one number
    f.shadow_pass(bias=0.0, pcf=1, ambient=AMBIENT, use_winner=False)
    want, lit = model(0.0, None)
    assert lit == 10703
    assert_bit_equal(host(f.get_color_tensor()), want, "bias 0 without the rule")
    f.render_arrays(s.tri, s.col, s.nrm, clear=True)
    f.shadow_pass(bias=1e-5, pcf=1, use_winner=False)
    assert model(1e-5, None)[1] == 15801
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "bias 1e-5 without the rule")


# ---- 3. odd shapes and the map's edge ------------------------------------------------------------------------------

def test_odd_shapes_and_the_maps_edge(oracle, odd_trex):
    s = odd_trex
    s.check([(1, True), (3, True), (5, True), (3, False)], "trex 200 x 173, map 96 x 80")
    counts = {}
    s.want(1, True, counts=counts)
    assert (counts["covered"], counts["lit"], counts["shadowed"]) == (7550, 3037, 4513)        # 40.2 % and 59.8 %
    # This light still sees the whole model (no texel of a covered pixel is off its map), so the edge is met by a
    # narrower one: at fov 12 the host model puts 59 % of the covered pixels off the map, where every tap is lit, and
    # the pixels along the edge have some of their taps outside
    assert s.off_the_map() == (0.0, 0.0)
    narrow = _Scene(oracle, (s.tri, s.col, s.nrm), 200, 173, 96, 80, s.R, s.t, light_fov=12.0)
    assert 0.5 < narrow.off_the_map()[0] < 0.7
    narrow.check([(1, True), (3, True), (5, False)], "trex 200 x 173, map 96 x 80, fov 12")


def test_a_row_strip_leaves_the_other_rows_alone(oracle, odd_trex):
    y0, y1 = 40, 136
    base = odd_trex
    s = _Scene(oracle, (base.tri, base.col, base.nrm), 200, 173, 96, 80, base.R, base.t, light_fov=30.0, y0=y0, y1=y1)
    f, g = s.fillers(camera_kw=dict(row_strip=(y0, y1)))
    for K in (1, 3, 5):
        s.draw(f, g)
        f.synchronize()
        # rows outside the strip: colours to be kept, and winners that WOULD be shadowed if the pass looked at them
        f.color_buffer[:y0] = 7.5
        f.color_buffer[y1:] = -2.25
        f.winner_buffer[:y0] = 0
        f.winner_buffer[y1:] = 1
        f.shadow_pass(bias=BIAS, pcf=K, ambient=AMBIENT)
        got = host(f.get_color_tensor())
        assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
        want = s.want(K, True, y0=y0, y1=y1)
        assert (want[y0:y1].view(np.uint32) != s.cam.color_buffer[y0:y1].view(np.uint32)).any()
        assert_bit_equal(got[y0:y1], want[y0:y1], f"strip rows, K={K}")


# ---- 4. behind the light -------------------------------------------------------------------------------------------

def test_a_model_partly_behind_the_light(oracle, odd_trex):
    base = odd_trex
    arrays = (base.tri, base.col, base.nrm)
    # t = (0, 0, -1.1) without the turn's own translation: the model stands beside this light, all of it off the map
    # and all but 7 of its 7 550 covered pixels behind the light, so the host model writes nothing
    s = _Scene(oracle, arrays, 200, 173, 96, 80, base.R, np.float32([0, 0, -1.1]), light_fov=30.0)
    off, behind = s.off_the_map()
    assert 0 < behind < 1 and abs(off + behind - 1) < 1e-9
    s.check([(1, True), (3, False), (5, True)], "behind the light", changes=False)
    assert_bit_equal(s.want(5, True), s.cam.color_buffer, "nothing is written")
    # the light INSIDE the model, one unit further along its axis than the turn puts it, with fov 90: the host model
    # has 27 % of the covered pixels behind the light, 24 % off the map, and shadows among the rest
    s = _Scene(oracle, arrays, 200, 173, 96, 80, base.R, (base.t + np.float32([0, 0, -1])).astype(np.float32), light_fov=90.0)
    off, behind = s.off_the_map()
    assert 0.2 < behind < 0.35 and 0.05 < off < 0.5
    counts = {}
    s.want(3, True, counts=counts)
    assert counts["shadowed"] > 0.2 * s.covered and counts["lit"] > 0.2 * s.covered
    s.check([(1, True), (3, True), (5, False)], "the light inside the model")


# ---- 5. random soups -----------------------------------------------------------------------------------------------

# what the host model leaves of the covered pixels at K = 1 with the winner rule: fully lit, fully shadowed
@pytest.mark.parametrize("seed,T,H,W,Hl,Wl,angles,kw,presort,lit,shadowed", [
    (51, 4000, 200, 173, 128, 128, (10, -20, 0), dict(size_px=(1.0, 40.0)), None, 26932, 7660),           # 77.9 %, 22.1 % of 34 592
    (52, 20000, 512, 509, 256, 192, (-15, 25, 5), dict(size_px=(2.0, 30.0)), True, 167792, 86119),        # 66.1 %, 33.9 % of 253 911
])
def test_random_soups(oracle, seed, T, H, W, Hl, Wl, angles, kw, presort, lit, shadowed):
    arrays = random_soup(np.random.default_rng(seed), T, max(H, W), **kw)
    s = _Scene(oracle, arrays, H, W, Hl, Wl, *shadow_ref.rotation_frame(arrays[0], angles))
    counts = {}
    s.want(1, True, counts=counts)
    assert (counts["lit"], counts["shadowed"]) == (lit, shadowed)
    assert min(lit, shadowed) >= 0.02 * counts["covered"]
    f, g = s.fillers(camera_kw=dict(presort=presort), light_kw=dict(presort=presort))
    s.check(EVERY, f"soup{seed}", f, g)
    if presort:
        # the resident inputs are the tile-coherent copies: the pass went through d_pos_of, and the light's winner
        # plane names the caller's triangles all the same
        assert f._order is not None and g._order is not None


# ---- 6. special values, through the C entry ------------------------------------------------------------------------

def _shade(lib, winner, tri, ltri, P, PL, lz, lwinner, color, bias=BIAS, ambient=AMBIENT, pcf=1, T=None, pos_of=None):
    import torch
    from cython3dmodelrenderer_amd import _capi
    T = tri.shape[0] if T is None else T
    H, W = winner.shape
    Hl, Wl = lz.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.crender_shadow_shade(
        winner.data_ptr(), tri.data_ptr() if T else None, T, None if pos_of is None else pos_of.data_ptr(), _capi.f32_16(P),
        ltri.data_ptr() if T else None, _capi.f32_16(PL), lz.data_ptr(), None if lwinner is None else lwinner.data_ptr(),
        Hl, Wl, bias, ambient, pcf, color.data_ptr(), H, W, 0, H, 0, st), "crender_shadow_shade")
    return host(color)


def test_special_values_through_the_c_entry(oracle):
    import torch
    from cython3dmodelrenderer_amd import _capi, shadow
    lib = _capi.load()
    rng = np.random.default_rng(61)
    H, W, Hl, Wl, T = 40, 37, 16, 16, 300
    tri, col, nrm = random_soup(rng, T, 40, size_px=(3.0, 25.0))
    ltri, lnrm = shadow.light_arrays(tri, nrm, *shadow_ref.rotation_frame(tri, (5, -10, 0)))
    cam = oracle.OracleFiller(H, W, fov=45.0)
    cam.render_arrays(tri, col, nrm)
    lig = oracle.OracleFiller(Hl, Wl, fov=45.0)
    lig.render_arrays(ltri, col, lnrm)
    assert (cam.winner >= 0).sum() > 500
    # the map: NaN, both infinities and the cleared 1e6 among the depths; light-frame corners that are NaN, infinite or
    # beyond int32 once projected; winners of both planes that name no triangle
    odd_z = np.float32([np.nan, np.inf, -np.inf, 1e6, -1e6, 0.0])
    lz = lig.z_buffer.copy()
    hit = rng.uniform(size=lz.shape) < 0.4
    lz[hit] = rng.choice(odd_z, int(hit.sum()))
    odd = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e12, -1e12, 0.0, -0.0])
    ltri = ltri.copy()
    hit = rng.uniform(size=ltri.shape) < 0.05
    ltri[hit] = rng.choice(odd, int(hit.sum()))
    bad = np.int32([-1, -2, T, T + 1, 2 ** 31 - 1, -2 ** 31])
    winner = cam.winner.copy()
    hit = rng.uniform(size=winner.shape) < 0.1
    winner[hit] = rng.choice(bad, int(hit.sum()))
    lwinner = lig.winner.copy()
    hit = rng.uniform(size=lwinner.shape) < 0.2
    lwinner[hit] = rng.choice(bad, int(hit.sum()))
    color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)

    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
           dict(winner=winner, tri=tri, ltri=ltri, lz=lz, lwinner=lwinner).items()}
    touched = 0
    for K in (1, 3, 5):
        for lw in (None, lwinner):
            for ambient in (AMBIENT, 0.0, 1.0):
                want = shadow_ref.shadow_pass(color, winner, tri, cam.proj_mat, ltri, lig.proj_mat, lz, lw, bias=BIAS,
                                              ambient=ambient, pcf=K)
                assert not np.isnan(want).any()              # every NaN is lit: none reaches the colours
                got = _shade(lib, dev["winner"], dev["tri"], dev["ltri"], cam.proj_mat, lig.proj_mat, dev["lz"],
                             None if lw is None else dev["lwinner"], torch.from_numpy(color).cuda(), ambient=ambient, pcf=K)
                assert_bit_equal(got, want, f"odd values, K={K}, winner={lw is not None}, ambient={ambient}")
                touched += int((want.view(np.uint32) != color.view(np.uint32)).any(2).sum())
                if ambient == 0.0 and K == 1:
                    assert (want == 0).all(2).sum() > 20      # fully shadowed pixels are black,
                if ambient == 1.0:
                    assert_bit_equal(want, color, "ambient 1")        # f = 1 + 0 * frac: written, with the same bits
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
    want = shadow_ref.shadow_pass(color, masked, tri, cam.proj_mat, ltri, lig.proj_mat, lz, lwinner, pcf=3)
    got = _shade(lib, dev["winner"], torch.from_numpy(moved).cuda(), dev["ltri"], cam.proj_mat, lig.proj_mat, dev["lz"],
                 dev["lwinner"], torch.from_numpy(color).cuda(), pcf=3, pos_of=torch.from_numpy(pos_of.view(np.int32)).cuda())
    assert_bit_equal(got, want, "d_pos_of with entries beyond T")
    # no triangles, and a frame that is background only: nothing is written
    for kw in (dict(T=0), dict()):
        w = dev["winner"] if kw else torch.full((H, W), -1, dtype=torch.int32).cuda()
        got = _shade(lib, w, dev["tri"], dev["ltri"], cam.proj_mat, lig.proj_mat, dev["lz"], dev["lwinner"],
                     torch.from_numpy(color).cuda(), pcf=5, **kw)
        assert_bit_equal(got, color, f"nothing to shade, {kw}")


# ---- 7. inputs and Renderer ----------------------------------------------------------------------------------------

def test_numpy_torch_and_device_model_inputs_agree(oracle):
    import torch
    from cython3dmodelrenderer_amd import scenes, shadow
    from cython3dmodelrenderer_amd.data_structures.device_model import DeviceModel
    from cython3dmodelrenderer_amd.data_structures.model import Model
    with np.load(os.path.join(GOLDEN, "trex_mesh.npz")) as z:
        m = Model(z["vertices"], z["faces"])
    scenes.fit_model(m)
    m.set_uniform_color()
    tri, col, nrm = m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles
    R, t = shadow.look_at((-0.8, -0.5, -0.2), tri.reshape(-1, 3).mean(0))
    s = _Scene(oracle, (tri, col, nrm), 256, 256, 192, 192, R, t)
    counts = {}
    want = s.want(3, True, counts=counts)
    assert counts["shadowed"] > 0.02 * s.covered and counts["lit"] > 0.02 * s.covered, counts

    f, g = s.fillers()                             # numpy
    s.draw(f, g)
    f.shadow_pass(pcf=3)
    assert_bit_equal(host(f.get_color_tensor()), want, "numpy inputs")

    f, g = s.fillers()                             # caller's device tensors, the light's arrays made on the device
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (tri, col, nrm)]
    dl, dn = shadow.light_arrays(dev[0], dev[2], R, t)
    assert dl.is_cuda
    assert_bit_equal(host(dl), s.ltri, "light_arrays on the device")
    f.render_arrays(*dev, clear=True)
    g.render_arrays(dl, dev[1], dn, clear=True)
    f.bind_shadow_map(g, dl)
    f.shadow_pass(pcf=3)
    assert_bit_equal(host(f.get_color_tensor()), want, "torch inputs")

    f, g = s.fillers()                             # the device-resident model
    dm = DeviceModel(m)
    f.render_model(dm, clear=True)
    dl, dn = shadow.light_arrays(dm._vertices_by_triangles, dm._normals_by_triangles, R, t)
    g.render_arrays(dl, dm._colors_by_triangles, dn, clear=True)
    f.bind_shadow_map(g, dl)
    f.shadow_pass(pcf=3)
    assert_bit_equal(host(f.get_color_tensor()), want, "DeviceModel inputs")
    # dropping the binding
    f.bind_shadow_map(None, None)
    with pytest.raises(ValueError, match="no shadow map is bound"):
        f.shadow_pass()


@pytest.fixture(scope="module")
def soup256(oracle):
    m = Soup()
    arrays = (m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles)
    s = _Scene(oracle, arrays, 256, 256, 128, 160, *shadow_ref.rotation_frame(arrays[0], (10, -20, 0)))
    s.model = m
    return s


@pytest.mark.parametrize("on_device", [None, False, True, "fused"])
def test_renderer_under_every_on_device(oracle, soup256, on_device):
    from cython3dmodelrenderer_amd.illumination.guro_illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    assert s.covered > 10000
    opts = dict(bias=2e-3, pcf=3, ambient=0.125, use_winner=True)
    if on_device == "fused":
        # the raster kernel shades as it stores, the pass multiplies what it finds
        lit = oracle.guro(s.cam.color_buffer.copy(), s.cam.normals_buffer, LIGHT)
        want = s.want(3, True, bias=2e-3, ambient=0.125, color=lit)
    else:
        want = oracle.guro(s.want(3, True, bias=2e-3, ambient=0.125), s.cam.normals_buffer, LIGHT)
    assert (want.view(np.uint32) != oracle.guro(s.cam.color_buffer.copy(), s.cam.normals_buffer, LIGHT).view(np.uint32)).any()
    f, g = s.fillers()
    r = Renderer(f, GuroIllumination(LIGHT), on_device=on_device, shadow=dict(filler=g, R=s.R, t=s.t, **opts))
    for _ in range(2):                             # every frame starts from cleared buffers: the same image twice
        out = r.render(s.model)
        got = host(out) if on_device in (True, "fused") else np.array(out)
        assert_bit_equal(got, want, f"Renderer(on_device={on_device!r}, shadow=...)")
    s.check_planes(f, g, "after Renderer")


def test_renderer_with_supersampling_and_with_a_texture_pass(oracle, soup256):
    from cython3dmodelrenderer_amd.data_structures.model import Model
    from cython3dmodelrenderer_amd.illumination.guro_illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = soup256
    light = GuroIllumination(LIGHT).light_direction
    # the pass runs on the supersampled frame, and the resolve carries the light over the shadowed colours
    f, g = s.fillers()
    r = Renderer(f, GuroIllumination(LIGHT), None, 128, 128, on_device=True, supersample=2, shadow=dict(filler=g, R=s.R, t=s.t, pcf=5))
    got = host(r.render(s.model))
    assert got.shape == (128, 128, 3)
    a, b = s.fillers()
    s.draw(a, b)
    a.shadow_pass(pcf=5)
    assert_bit_equal(host(a.get_color_tensor()), s.want(5, True), "the supersampled frame, shadowed")
    assert_bit_equal(host(f.get_color_tensor()), s.want(5, True), "the Renderer's frame stays unshaded")
    assert_bit_equal(got, host(a.resolve(2, light_direction=light)), "Renderer(supersample=2, shadow=...)")
    # after a texture pass: the shadow falls on the texture's colours
    rng = np.random.default_rng(72)
    T = len(s.tri)
    idx = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    uv = rng.uniform(0, 1, (T, 3, 2)).astype(np.float32)
    tex = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    m = Model(s.tri.reshape(-1, 3), idx, uv.reshape(-1, 2), idx, tex, s.nrm.reshape(-1, 3), idx, recalculate_normals=False)
    assert_bit_equal(m._vertices_by_triangles, s.tri, "the model's triangles")
    assert_bit_equal(m._normals_by_triangles, s.nrm, "the model's normals")
    f, g = s.fillers()
    r = Renderer(f, GuroIllumination(LIGHT), on_device=True, texture_pass={"perspective": True}, shadow=dict(filler=g, R=s.R, t=s.t))
    got = host(r.render(m))
    a, b = s.fillers()
    a.bind_texture(m.get_texture_coords_by_triangles(), tex)
    a.render_model(m, clear=True)
    a.texture_pass(perspective=True)
    textured = host(a.get_color_tensor())
    want = oracle.guro(s.want(1, True, color=textured), s.cam.normals_buffer, LIGHT)
    assert_bit_equal(got, want, "Renderer(texture_pass=..., shadow=...)")


def test_host_views_show_the_shadowed_colours_at_the_next_getter_call(soup256):
    s = soup256
    f, g = s.fillers()
    s.draw(f, g)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    f.shadow_pass()
    again = f.get_color_buffer()
    assert again is view
    assert_bit_equal(view, s.want(), "after the pass")
    # an edit of the light's z view reaches the pass: a map moved to the far plane shadows nothing
    s.draw(f, g)
    z = g.get_z_buffer()
    z[:] = 1e6
    f.shadow_pass(use_winner=False)
    assert_bit_equal(f.get_color_buffer(), s.cam.color_buffer, "under an emptied map")


def test_errors_name_their_cause(soup256):
    from cython3dmodelrenderer_amd import _capi
    s = soup256
    f, g = s.fillers(camera_kw=dict(track_winner=False))
    s.draw(f, g)
    with pytest.raises(ValueError, match="winner plane"):
        f.shadow_pass()
    f, g = s.fillers()
    with pytest.raises(ValueError, match="no shadow map is bound"):
        f.shadow_pass()
    f.bind_shadow_map(g, s.ltri)
    with pytest.raises(ValueError, match="no frame has been rendered by the camera's filler"):
        f.shadow_pass()
    f.render_arrays(s.tri, s.col, s.nrm, clear=True)
    with pytest.raises(ValueError, match="no frame has been rendered by the light's filler"):
        f.shadow_pass()
    g.render_arrays(s.ltri[:-1], s.col[:-1], s.lnrm[:-1], clear=True)
    with pytest.raises(ValueError, match="3000 triangles of light-frame vertices are bound, the light's last frame drew 2999, "
                                         "the camera's 3000"):
        f.shadow_pass()
    g.render_arrays(s.ltri, s.col, s.lnrm, clear=True)
    f.bind_shadow_map(g, s.ltri[:-1])
    with pytest.raises(ValueError, match="2999 triangles of light-frame vertices are bound"):
        f.shadow_pass()
    f.bind_shadow_map(g, s.ltri)
    g.render_arrays(s.ltri, s.col, s.lnrm)         # composites on the frame before
    with pytest.raises(ValueError, match="the light's filler did not start from cleared buffers"):
        f.shadow_pass()
    g.render_arrays(s.ltri, s.col, s.lnrm, clear=True)
    f.render_arrays(s.tri, s.col, s.nrm)
    with pytest.raises(ValueError, match="the camera's filler did not start from cleared buffers"):
        f.shadow_pass()
    f.render_arrays(s.tri, s.col, s.nrm, clear=True)
    for pcf in (0, 2, 7, True, 3.0 + 0.5):
        with pytest.raises(ValueError, match="pcf must be 1, 3 or 5"):
            f.shadow_pass(pcf=pcf)
    with pytest.raises(_capi.CrenderError, match="ambient outside"):
        f.shadow_pass(ambient=1.5)
    with pytest.raises(_capi.CrenderError, match="bias is not finite"):
        f.shadow_pass(bias=float("nan"))
    f.shadow_pass()                                # and works again
    assert_bit_equal(host(f.get_color_tensor()), s.want(), "after the errors")
    # a light filler without a winner plane: use_winner=True falls back to the depths alone
    g2 = filler(s.Hl, s.Wl, track_winner=False)
    f.render_arrays(s.tri, s.col, s.nrm, clear=True)
    g2.render_arrays(s.ltri, s.col, s.lnrm, clear=True)
    f.bind_shadow_map(g2, s.ltri)
    f.shadow_pass(use_winner=True)
    assert_bit_equal(host(f.get_color_tensor()), s.want(1, False), "a light without a winner plane")
    for bad in ((None, s.ltri), (g, None), (object(), s.ltri), (g, s.ltri.astype(np.float64)), (g, s.ltri[:, :, :2])):
        with pytest.raises(ValueError):
            f.bind_shadow_map(*bad)
    with pytest.raises(ValueError, match="swap chain"):
        f.bind_shadow_map(filler(64, 64, pipeline=True), s.ltri)
    chain = filler(64, 64, pipeline=True)
    chain.bind_shadow_map(g, s.ltri)
    with pytest.raises(ValueError, match="swap chain"):
        chain.shadow_pass()


# ---- 8. bin overflow -----------------------------------------------------------------------------------------------

def test_a_frame_redrawn_after_a_bin_overflow_ends_shadowed(oracle):
    """The scene of test_filler_recovers_from_bin_overflow: the bin lists are far too small, the frame drops fragments
    and is rendered again when it is settled — which the pass does, for the camera's frame and for the light's, before
    it launches."""
    arrays = random_soup(np.random.default_rng(21), 400, 512, size_px=(150, 400), frac_backface=0.0)
    s = _Scene(oracle, arrays, 512, 512, 512, 512, *shadow_ref.rotation_frame(arrays[0], (5, -10, 0)))
    counts = {}
    want = s.want(3, True, counts=counts)
    assert counts["shadowed"] > 0.02 * s.covered and counts["lit"] > 0.02 * s.covered, counts
    small = dict(tile=32, bin_capacity=500, direct_bins=False)
    for camera_kw, light_kw in ((small, None), (None, small), (dict(small, presort=True), dict(small, presort=True))):
        f, g = s.fillers(camera_kw, light_kw)
        s.draw(f, g)
        for filler, kw in ((f, camera_kw), (g, light_kw)):
            if kw:
                need, cap = filler.bin_usage()
                assert cap == 500 and need > cap and len(filler._pending) == 1     # dropped fragments, nobody has looked yet
        f.shadow_pass(pcf=3)
        assert not f._pending and not g._pending                                   # grown and redone before the pass
        assert_bit_equal(host(f.get_color_tensor()), want, f"redone frames, {camera_kw}, {light_kw}")
        s.check_planes(f, g, "redone frames")
