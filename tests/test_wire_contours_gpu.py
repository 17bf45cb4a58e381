"""The contour edges on the GPU (csrc/wireframe.hip's k_wire_facing and k_wire_contour_mask through
AdvancedPixelBufferFiller.contour_edges, the C entry and Renderer(wireframe={"contours": True, ...})), bit for bit
against the host model of tests/contour_ref.py (itself pinned in tests/test_wire_contours_cpu.py); and the frames drawn
from its masks against tests/outline_ref.py on the oracle's frames."""
import ctypes as C

import numpy as np
import pytest

import contour_ref
import outline_ref
from pass_scenes import Scene, TriangleModel, filler, host, lib, trex_fixture  # noqa: F401 (fixtures)
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)              # what GuroIllumination is constructed with
LINE = (250.0, 240.0, 20.0)
FILL = (30.0, 35.0, 40.0)
H, W = 96, 160                       # the generated meshes' frame: not square
POSES = ((0, 0, 0), (25, 40, 10), (-70, 15, 200))


def _partners(tri):
    from cython3dmodelrenderer_amd.wireframe import edge_partners
    return edge_partners(tri)


def _static(tri, angle=30.0):
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    return feature_edges(tri, angle)


class _Scene(Scene):
    """A scene with its partner table; ``want_mask`` is the model's mask of the oracle's view."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.partners = _partners(self.tri)

    def want_mask(self, static=None, borders=False, partners=None):
        return contour_ref.contour_edges(self.tri, self.cam.proj_mat, self.W, self.H,
                                         self.partners if partners is None else partners, static, borders)[0]

    def want(self, edges, base=None, **kw):
        """The model's frame after ``wire_pass(outline=True, edges=edges, **kw)`` over `base` (the oracle's colours if
        None); -> (colours, counts)."""
        kw = dict(kw)
        kw["line"] = kw.pop("color", kw.pop("line", (255, 255, 255)))
        counts = {}
        out = outline_ref.wire_pass(self.cam.color_buffer if base is None else base, self.cam.winner, self.cam.z_buffer,
                                    self.tri, self.cam.proj_mat, edges=edges, counts=counts, **kw)
        return out, counts


trex256 = trex_fixture(_Scene)


@pytest.fixture(scope="module")
def spheres(oracle):
    """The generated sphere at three poses, 96 x 160."""
    out = []
    for angles in POSES:
        tri = contour_ref.place(contour_ref.uv_sphere(), angles)
        out.append(_Scene(oracle, (tri,) + contour_ref.attributes(tri), H, W))
        assert out[-1].covered > 5000
    return out


# ---- 1. the mask is the model's --------------------------------------------------------------------------------------

def test_trex_masks(trex256):
    s = trex256
    f = filler(256, 256)
    s.draw(f)
    static = _static(s.tri) | np.uint8(0xA8)          # bits 3 to 7 of a static mask are ignored, and written 0
    for st in (None, static):
        for borders in (False, True):
            got = f.contour_edges(s.partners, static=st, borders=borders)
            assert str(got.dtype) == "torch.uint8" and got.is_cuda and tuple(got.shape) == (len(s.tri),)
            assert_bit_equal(host(got), s.want_mask(st, borders), f"T-Rex, static {st is not None}, borders {borders}")
    plain = host(f.contour_edges(s.partners))
    assert int(np.unpackbits(plain).sum()) == 4810 and not (host(got) >> 3).any()
    assert (plain != (static & 7)).any()
    s.check_planes(f, "T-Rex after contour_edges")   # nothing but the mask was written
    assert_bit_equal(host(f.get_color_tensor()), s.cam.color_buffer, "the colours are not touched")


def test_the_sphere_in_a_frame_that_is_not_square(spheres):
    f = filler(H, W)
    masks = []
    for s, angles in zip(spheres, POSES):
        s.draw(f)
        for borders in (False, True):
            got = host(f.contour_edges(s.partners, borders=borders))
            assert_bit_equal(got, s.want_mask(None, borders), f"sphere at {angles}, borders {borders}")
        assert got.any()
        masks.append(got)
    assert (masks[0] != masks[1]).any() and (masks[1] != masks[2]).any()


@pytest.mark.parametrize("T", [1, 2, 255, 256, 257])
def test_cuts_of_the_sphere(oracle, T):
    """The seams of the workgroups, and a table whose partners point past T: they are no partners."""
    tri = contour_ref.place(contour_ref.uv_sphere(), POSES[1])[:T]
    col, nrm = contour_ref.attributes(tri)
    partners = _partners(contour_ref.place(contour_ref.uv_sphere(), POSES[1]))[:T]
    assert T >= 256 or ((partners >> 1) >= T).any()
    P = oracle.OracleFiller(H, W, fov=45.0).proj_mat
    static = np.random.default_rng(T).integers(0, 256, T).astype(np.uint8)
    f = filler(H, W)
    f.render_arrays(tri, col, nrm, clear=True)
    for st in (None, static):
        for borders in (False, True):
            got = host(f.contour_edges(partners, static=st, borders=borders))
            want = contour_ref.contour_edges(tri, P, W, H, partners, st, borders)[0]
            assert_bit_equal(got, want, f"T = {T}, static {st is not None}, borders {borders}")
            assert not (got >> 3).any()
    # and with the cut's own table every open edge is a border
    own = _partners(tri)
    got = host(f.contour_edges(own, borders=True))
    assert_bit_equal(got, contour_ref.contour_edges(tri, P, W, H, own, None, True)[0], f"T = {T}, its own table")
    assert T > 2 or (got == 7).all()


def test_a_presorted_filler_gives_the_caller_s_order(spheres, trex256):
    for s, size in ((spheres[1], (H, W)), (trex256, (256, 256))):
        plain, sorted_ = filler(*size), filler(*size, presort=True)
        static = np.random.default_rng(4).integers(0, 8, len(s.tri)).astype(np.uint8)
        s.draw(plain)
        s.draw(sorted_)
        assert plain._order is None and sorted_._order is not None     # the pass goes through d_pos_of
        a, b = host(plain.contour_edges(s.partners, static=static)), host(sorted_.contour_edges(s.partners, static=static))
        assert_bit_equal(b, a, "presort=True against the same mesh unsorted")
        assert_bit_equal(a, s.want_mask(static), "and both are the model's")
    perm = host(sorted_._order[1]).astype(np.int64)
    assert (perm != np.arange(len(perm))).any()                         # T-Rex's resident order is not the caller's


# ---- 2. hostile corners and tables, through the C entry -------------------------------------------------------------

def _contours(lib, tri, P, partners, Hh, Ww, static=None, flags=0, pos_of=None, T=None):
    import torch
    from cython3dmodelrenderer_amd import _capi
    T = tri.shape[0] if T is None else T
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (tri, partners, static, pos_of)]
    facing = torch.full((max(T, 1),), 99, dtype=torch.int8, device="cuda")
    edges = torch.full((max(T, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.crender_wire_contours(dev[0].data_ptr() if T else None, T, None if dev[3] is None else dev[3].data_ptr(),
                                          _capi.f32_16(P), dev[1].data_ptr(), None if dev[2] is None else dev[2].data_ptr(),
                                          facing.data_ptr(), edges.data_ptr(), Hh, Ww, flags, st), "crender_wire_contours")
    assert_bit_equal(host(dev[0]), np.ascontiguousarray(tri), "the triangles are only read")
    return host(edges), host(facing)


def test_hostile_corners_and_junk_tables_through_the_c_entry(oracle, lib):
    P = oracle.OracleFiller(H, W, fov=45.0).proj_mat
    rng = np.random.default_rng(17)
    tri = contour_ref.place(contour_ref.uv_sphere(), POSES[1])
    T = len(tri)
    partners = _partners(tri)
    # corners at NaN, at infinities, at z = 0, behind the camera; two equal corners; three corners on one projected line
    odd = np.float32([np.nan, np.inf, -np.inf, 0.0, -0.0, 3e38, -3e38])
    hit = rng.uniform(size=tri.shape) < 0.04
    tri[hit] = rng.choice(odd, int(hit.sum()))
    tri[5:25, 1, 2] = 0.0                                # z = 0: the projection divides by it
    tri[30:50, :, 2] *= -1.0                             # behind the camera: projected as the rasterizer projects it
    tri[60:70, 2] = tri[60:70, 0]                        # two equal corners: no area
    for k, z in enumerate((2.0, 4.0, 8.0)):              # on one line through the image's centre
        tri[80 + k] = np.float32([[-0.5, -0.25, 1.0], [0.0, 0.0, 1.0], [0.5, 0.25, 1.0]]) * np.float32(z)
    for flags in (0, 1):
        got, facing = _contours(lib, tri, P, partners, H, W, flags=flags)
        want, face = contour_ref.contour_edges(tri, P, W, H, partners, borders=bool(flags))
        assert_bit_equal(facing, face, f"facing of hostile corners, flags {flags}")
        assert_bit_equal(got, want, f"mask of hostile corners, flags {flags}")
    assert (face[60:70] == 0).all() and (face[80:83] == 0).all() and (face == 0).sum() > 30
    assert (face == 1).sum() > 40 and (face == -1).sum() > 40 and got.any()
    # a junk table: nothing in it is used as an index but what lies below T
    junk = np.int32([-3, -4, 2 * T, 2 * T + 1, 2 ** 31 - 1, 2 ** 31 - 2, -2 ** 31, -1, -2])
    table = partners.copy()
    hit = rng.uniform(size=table.shape) < 0.5
    table[hit] = rng.choice(junk, int(hit.sum()))
    static = rng.integers(0, 256, T).astype(np.uint8)
    for flags in (0, 1):
        for st in (None, static):
            got, facing = _contours(lib, tri, P, table, H, W, static=st, flags=flags)
            assert_bit_equal(got, contour_ref.mask(face, table, st, flags), f"a junk table, flags {flags}, static {st is not None}")
            assert_bit_equal(facing, face, "the facing does not depend on the table")
    only = np.full((T, 3), 2 ** 31 - 1, np.int32)
    for junk_value in (-3, 2 * T, 2 ** 31 - 1):
        only[:] = junk_value
        assert not _contours(lib, tri, P, only, H, W, flags=1)[0].any(), junk_value
    # d_pos_of: the triangles elsewhere, some of them nowhere
    perm = rng.permutation(T).astype(np.uint32)
    moved = np.empty_like(tri)
    moved[perm] = tri
    pos_of = perm.copy()
    gone = rng.uniform(size=T) < 0.3
    pos_of[gone] = rng.choice(np.uint32([T, T + 7, 2 ** 32 - 1]), int(gone.sum()))
    got, facing = _contours(lib, moved, P, partners, H, W, static=static, flags=1, pos_of=pos_of.view(np.int32))
    want, face2 = contour_ref.contour_edges(moved, P, W, H, partners, static, True, pos_of)
    assert not face2[gone].any() and (face2[~gone] == face[~gone]).all()
    assert_bit_equal(facing, face2, "facing through d_pos_of")
    assert_bit_equal(got, want, "mask through d_pos_of")
    # no triangles: nothing is written
    got, facing = _contours(lib, tri, P, partners, H, W, T=0)
    assert (got == 0xEE).all() and (facing == 99).all()


# ---- 3. the table made on the device ---------------------------------------------------------------------------------

def test_edge_partners_on_the_device(trex256):
    import torch
    tri, want = contour_ref.hand_mesh()
    for mesh, table in ((tri, want), (trex256.tri, trex256.partners)):
        got = _partners(torch.from_numpy(mesh).cuda())
        assert got.is_cuda and got.dtype == torch.int32
        assert_bit_equal(host(got), table, f"edge_partners of {len(mesh)} triangles on the device")


# ---- 4. end to end ---------------------------------------------------------------------------------------------------

WIRE = dict(width=1.0, color=LINE, fill=FILL, outline=True)


def _check_frame(s, f, partners, static, what, **wire):
    """contour_edges and wire_pass on the frame `f` holds; the colours are the model's under the model's mask."""
    mask = f.contour_edges(partners, static=static, borders=True)
    want_mask = s.want_mask(static if static is None or isinstance(static, np.ndarray) else host(static), True)
    assert_bit_equal(host(mask), want_mask, f"{what}: mask")
    f.wire_pass(edges=mask, **wire)
    kw = {k: v for k, v in wire.items() if k != "outline"}
    want, counts = s.want(want_mask, **kw)
    assert_bit_equal(host(f.get_color_tensor()), want, f"{what}: colour")
    s.check_planes(f, what)
    return host(mask), counts, kw


def test_end_to_end_on_trex_and_the_sphere(trex256, spheres):
    for s, size, angle, name in ((trex256, (256, 256), 30.0, "T-Rex"), (spheres[1], (H, W), 15.0, "sphere")):
        f = filler(*size)
        static = _static(s.tri, angle)
        s.draw(f)
        mask, counts, kw = _check_frame(s, f, s.partners, static, name, **WIRE)
        assert (mask != static).any()                                   # the view adds edges to the static mask
        without = s.want(static, **kw)[1]
        assert counts["background_on"] > without["background_on"], (name, counts, without)
        if name == "T-Rex":
            assert (without["background_on"], counts["background_on"]) == (583, 745)
            assert (without["covered_on"], counts["covered_on"]) == (4250, 4454)


def test_a_session_of_a_device_model(oracle):
    """One filler, five poses of one DeviceModel turned on the device; the table once, on the device; the mask per pose."""
    import torch
    from cython3dmodelrenderer_amd.data_structures.device_model import DeviceModel
    m = DeviceModel(contour_ref.sphere_model())
    f = filler(H, W)
    partners = _partners(m._vertices_by_triangles)
    assert isinstance(partners, torch.Tensor) and partners.is_cuda
    static = torch.from_numpy(_static(host(m._vertices_by_triangles), 15.0)).cuda()
    back, there = -np.float32(contour_ref.CENTRE), np.float32(contour_ref.CENTRE)
    masks = []
    for pose in range(5):
        if pose:
            m.shift(back)
            m.rotate((17, 9, 5))
            m.shift(there)
        f.render_model(m, clear=True)
        arrays = tuple(host(a) for a in (m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles))
        s = _Scene(oracle, arrays, H, W)
        assert s.covered > 5000
        # the table made before the first pose is the table of every pose: equal vertices turn into equal vertices
        assert_bit_equal(host(partners), s.partners, f"pose {pose}: the table")
        mask, counts, _ = _check_frame(s, f, partners, static, f"pose {pose}", **WIRE)
        assert counts["background_on"] > 0
        masks.append(mask)
    assert sum((a != b).any() for a, b in zip(masks, masks[1:])) >= 2


# ---- 5. Renderer -----------------------------------------------------------------------------------------------------

OPTS = dict(contours=True, feature_angle=15, outline=True, fill=FILL, color=LINE)


def _by_hand(a, model, tri, shade, borders=True, contours=True):
    """The passes a Renderer with OPTS runs, called one by one on the filler `a`."""
    a.set_fused_illumination(None)
    a.render_model(model, clear=True)
    shade(a)
    edges = _static(tri, 15.0)
    if contours:
        edges = a.contour_edges(_partners(tri), static=edges, borders=borders)
    a.wire_pass(outline=True, fill=FILL, color=LINE, edges=edges)


def test_renderer_draws_the_contours(spheres):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = spheres[1]
    model = TriangleModel(s.tri, s.col, s.nrm)
    guro = GuroIllumination(GURO)
    phong = PhongIllumination(position=(0.3, -0.2, 0.0), ambient=0.2)
    cases = (("Guro on the device", guro, dict(on_device=True)), ("Guro, the default", guro, dict(on_device=None)),
             ("Phong", phong, dict(on_device=True)))
    frames = {}
    for name, ill, kw in cases:
        f, a = filler(H, W), filler(H, W)
        got = Renderer(f, ill, wireframe=OPTS, **kw).render(model)
        got = got if isinstance(got, np.ndarray) else host(got)
        _by_hand(a, model, s.tri, ill.draw_illumination_device)
        assert_bit_equal(got, host(a.get_color_tensor()), f"{name}: the Renderer against the passes by hand")
        frames[name] = got
        s.check_planes(f, name)
    # anchored on the model: under Guro the lit colours are what the lines are blended over, the fill covers the body
    b = filler(H, W)
    b.render_model(model, clear=True)
    guro.draw_illumination_device(b)
    lit = host(b.get_color_tensor()).copy()
    mask = s.want_mask(_static(s.tri, 15.0), True)
    want, counts = s.want(mask, base=lit, line=LINE, fill=FILL)
    assert counts["background_on"] > 0
    assert_bit_equal(frames["Guro on the device"], want, "the Renderer against the model")
    assert_bit_equal(frames["Guro, the default"], want, "the Renderer's numpy view against the model")
    # the keys reach the pass: no borders is the same on a closed mesh, no contours is not
    f = filler(H, W)
    closed = host(Renderer(f, guro, on_device=True, wireframe=dict(OPTS, borders=False)).render(model))
    assert_bit_equal(closed, want, "borders=False on a closed mesh")
    # supersampled: the lines on the large frame, then the resolve
    f, a = filler(H, W), filler(H, W)
    got = host(Renderer(f, guro, None, H // 2, W // 2, on_device=True, supersample=2, wireframe=OPTS).render(model))
    assert got.shape == (H // 2, W // 2, 3)
    _by_hand(a, model, s.tri, guro.draw_illumination_device)
    assert_bit_equal(host(f.get_color_tensor()), want, "the supersampled frame is the model's")
    assert_bit_equal(got, host(a.resolve(2)), "supersample=2: the Renderer against the passes by hand")


def test_renderer_without_contours_is_the_parent_s(spheres):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    s = spheres[1]
    model = TriangleModel(s.tri, s.col, s.nrm)
    guro = GuroIllumination(GURO)
    opts = {k: v for k, v in OPTS.items() if k != "contours"}
    f, a = filler(H, W), filler(H, W)
    r = Renderer(f, guro, on_device=True, wireframe=opts)
    got = host(r.render(model))
    _by_hand(a, model, s.tri, guro.draw_illumination_device, contours=False)
    assert_bit_equal(got, host(a.get_color_tensor()), "without contours: feature_edges and wire_pass by hand")
    a.render_model(model, clear=True)
    guro.draw_illumination_device(a)
    lit = host(a.get_color_tensor()).copy()
    assert_bit_equal(got, s.want(_static(s.tri, 15.0), base=lit, line=LINE, fill=FILL)[0], "and the model under the static mask")
    assert r._wired[2] is None
    with_contours = host(Renderer(filler(H, W), guro, on_device=True, wireframe=OPTS).render(model))
    assert (with_contours != got).any()


def test_renderer_with_a_device_model_keeps_everything_on_the_device(oracle):
    """The table is made from the model's device tensor and handed on as one; the frame is that of the host's arrays."""
    import torch
    from cython3dmodelrenderer_amd.data_structures.device_model import DeviceModel
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    host_model = contour_ref.sphere_model()
    m = DeviceModel(host_model)
    guro = GuroIllumination(GURO)
    f = filler(H, W)
    r = Renderer(f, guro, on_device=True, wireframe=OPTS)
    got = host(r.render(m))
    table = r._wired[2]
    assert isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.int32
    tri = host_model._vertices_by_triangles
    assert_bit_equal(host(table), _partners(tri), "the device model's table")
    a = filler(H, W)
    _by_hand(a, host_model, tri, guro.draw_illumination_device)
    assert_bit_equal(got, host(a.get_color_tensor()), "a DeviceModel against the host model's arrays")
    r.render(m)
    assert r._wired[2] is table                        # once per model


# ---- 6. errors -------------------------------------------------------------------------------------------------------

def test_errors_name_their_cause(spheres):
    s = spheres[0]
    T = len(s.tri)
    f = filler(H, W)
    with pytest.raises(ValueError, match="contour_edges: no frame has been rendered"):
        f.contour_edges(s.partners)
    with pytest.raises(ValueError, match="swap chain"):
        filler(64, 64, pipeline=True).contour_edges(s.partners)
    s.draw(f)
    with pytest.raises(ValueError, match=rf"holds {T - 1} triangles, the last frame drew {T}"):
        f.contour_edges(s.partners[:-1])
    with pytest.raises(ValueError, match=rf"holds {T + 1} triangles, the last frame drew {T}"):
        f.contour_edges(s.partners, static=np.zeros(T + 1, np.uint8))
    with pytest.raises(ValueError, match="int32"):
        f.contour_edges(s.partners.astype(np.int64))
    # it needs no winner plane
    g = filler(H, W, track_winner=False)
    s.draw(g)
    assert_bit_equal(host(g.contour_edges(s.partners)), s.want_mask(), "a filler without a winner plane")
