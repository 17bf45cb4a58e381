"""Geometric edge anti-aliasing on the GPU (csrc/wireframe.hip's k_wire_edge_aa through AdvancedPixelBufferFiller.edge_aa,
the C entry and Renderer(antialias=...)), bit for bit against the host model of tests/edge_aa_ref.py evaluated on the
oracle's frames and on painted planes (itself pinned in tests/test_edge_aa_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import contour_ref
import edge_aa_ref
import pass_edges as E
from pass_scenes import Scene, edge_mask, filler, host, lib, soup_fixture, textured_model, trex_arrays, trex_fixture  # noqa: F401
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)              # what GuroIllumination is constructed with
LINE = (250.0, 240.0, 20.0)


class _Scene(Scene):
    def want(self, base=None, **kw):
        """The model's plane over `base` (the oracle's colours if None)."""
        return edge_aa_ref.edge_aa(self.cam.color_buffer if base is None else base, self.cam.winner, self.cam.z_buffer,
                                   self.tri, None, self.cam.proj_mat, **kw)[0]

    def check(self, f, what, edges=None, model_edges=None):
        """Draw, run the pass with `edges` and compare with the model under `model_edges` (`edges` itself if None)."""
        self.draw(f)
        out = f.edge_aa(edges=edges)
        want = self.want(edges=edges if model_edges is None else model_edges)
        changed = self.assert_changed(want, what)
        assert tuple(out.shape) == (self.H, self.W, 3) and out.data_ptr() != f.color_buffer.data_ptr()
        assert_bit_equal(host(out), want, f"{what}: the result")
        assert_bit_equal(host(f.get_color_tensor()), self.cam.color_buffer, f"{what}: the colour plane is only read")
        self.check_planes(f, what)
        return want, changed


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


# ---- 1. T-Rex and the soup at 256 x 256, every kind of mask -----------------------------------------------------------

@pytest.mark.parametrize("scene", ["trex", "soup"])
def test_every_mask(trex256, soup256, scene):
    import torch
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    s = trex256 if scene == "trex" else soup256
    f = filler(256, 256)
    all_edges, _ = s.check(f, f"{scene}, all edges")
    for kind in ("random", "feature"):
        mask = edge_mask(kind, s.tri)
        want, _ = s.check(f, f"{scene}, {kind} mask", edges=mask)
        assert kind == "feature" or (want != all_edges).any()            # (every edge of a soup is a border: its feature mask is full)
    # the mask of the view, classified on the device and handed over as the device tensor it is
    s.draw(f)
    static = feature_edges(s.tri, 30.0)
    view = f.contour_edges(edge_partners(s.tri), static=static, borders=True)
    assert isinstance(view, torch.Tensor) and view.is_cuda
    want_view = contour_ref.contour_edges(s.tri, s.cam.proj_mat, 256, 256, edge_partners(s.tri), static=static, borders=True)[0]
    assert np.array_equal(host(view), want_view)
    want, changed = s.check(f, f"{scene}, the contours of the view", edges=view, model_edges=want_view)
    if scene == "trex":              # (every edge of a soup is a border: its mask is full again)
        assert (want != all_edges).any() and changed.sum() < (all_edges != s.cam.color_buffer).any(2).sum()
    # an all-zero mask copies the plane
    s.draw(f)
    assert_bit_equal(host(f.edge_aa(edges=np.zeros(len(s.tri), np.uint8))), s.cam.color_buffer, f"{scene}, no edge smooths")


# ---- 2. the edges of the tiles, the halo and the strip --------------------------------------------------------------

def _edge_aa(lib, winner, z, tri, P, color, edges=None, T=None, pos_of=None, y0=0, y1=None, out=None):
    """crender_wire_edge_aa on numpy planes: the result plane (rows outside y0 .. y1 are `out`'s, NaN without one)."""
    import torch
    from cython3dmodelrenderer_amd import _capi
    H, W = winner.shape
    T = tri.shape[0] if T is None else T
    y1 = H if y1 is None else y1
    pos_of = None if pos_of is None else np.ascontiguousarray(pos_of).view(np.int32)      # (the same 32 bits)
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (winner, z, tri, pos_of, edges, color)]
    d_out = torch.from_numpy(np.full((H, W, 3), np.nan, np.float32) if out is None else np.ascontiguousarray(out)).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = [None if a is None else a.data_ptr() for a in dev]
    _capi.check(lib.crender_wire_edge_aa(ptr[0], ptr[1], ptr[2] if T else None, T, ptr[3], _capi.f32_16(P), ptr[4],
                                         d_out.data_ptr(), ptr[5], H, W, y0, y1, 0, st), "crender_wire_edge_aa")
    got = host(d_out)
    for a, b, name in zip(dev, (winner, z, tri, pos_of, edges, color), ("winner", "z", "tri", "pos_of", "edges", "colour")):
        if a is not None:
            assert_bit_equal(host(a), np.ascontiguousarray(b), f"{name} is only read")
    return got


def _model(winner, z, tri, P, color, edges=None, pos_of=None, y0=0, y1=None, out=None):
    H, W = winner.shape
    start = np.full((H, W, 3), np.nan, np.float32) if out is None else out
    return edge_aa_ref.edge_aa(color, winner, z, tri, pos_of, P, edges=edges, y0=y0, y1=y1, out=start)


def _painted(H, W, seed, T=14):
    """Planes no rasterizer makes, for a frame of any shape: triangles across the frame, a winner plane painted in runs
    of a few pixels with background and winners beyond T among them, random depths with ties, random colours."""
    rng = np.random.default_rng(seed)
    sx = rng.uniform(-12, W + 12, (T, 3))
    sy = rng.uniform(-12, H + 12, (T, 3))
    tri = np.ascontiguousarray(E.unproject(sx, sy, rng.uniform(0.6, 2.5, (T, 3)), W, H))
    coarse = rng.integers(-1, T + 2, ((H + 2) // 3, (W + 3) // 4)).astype(np.int32)
    winner = np.repeat(np.repeat(coarse, 3, 0), 4, 1)[:H, :W].copy()
    hit = rng.uniform(size=winner.shape) < 0.15
    winner[hit] = rng.integers(-1, T, int(hit.sum()))
    z = rng.choice(np.float32([0.5, 0.625, 0.75, 0.875]), (H, W))
    color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    mask = rng.integers(0, 256, T).astype(np.uint8)
    return winner, z, tri, color, mask


@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (70, 1), (33, 33), (84, 100)])
def test_frames_that_do_not_fit_the_tiles(lib, oracle, H, W):
    """Not multiples of 32: the halo falls off every side, the last tile is partial both ways, a frame is one pixel."""
    winner, z, tri, color, mask = _painted(H, W, 1000 * H + W)
    blended = 0
    for edges in (None, mask):
        want, a, _ = _model(winner, z, tri, E.P, color, edges=edges)
        assert_bit_equal(_edge_aa(lib, winner, z, tri, E.P, color, edges=edges), want, f"{H} x {W}, painted, mask {edges is not None}")
        assert not np.isnan(want).any()
        blended += int((a > 0).sum())
    assert blended >= (0 if H * W == 1 else 10)
    if min(H, W) > 1:
        # and rasterized, through the filler
        s = _Scene(oracle, random_soup(np.random.default_rng(H), 300, max(H, W), size_px=(3.0, 25.0)), H, W)
        assert s.covered > 100
        s.check(filler(H, W), f"{H} x {W}, a soup")


def test_a_row_strip_that_starts_and_ends_inside_a_tile(lib, oracle):
    y0, y1 = 40, 136
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    s.draw(f)
    f.synchronize()
    # rows outside the strip: colours that must not be read, and winners that WOULD smooth if the pass looked at them
    f.color_buffer[:y0] = 7.5
    f.color_buffer[y1:] = -2.25
    f.winner_buffer[:y0] = 0
    f.winner_buffer[y1:] = 1
    got = host(f.edge_aa())
    assert not got[:y0].any() and not got[y1:].any()                     # the filler's rows; the others stay zero
    want = s.want(y0=y0, y1=y1)
    assert (want[y0:y1].view(np.uint32) != s.cam.color_buffer[y0:y1].view(np.uint32)).any()
    assert_bit_equal(got[y0:y1], want[y0:y1], "the strip's rows")
    whole = _Scene(oracle, trex_arrays(), 200, 173).want()
    assert (whole[y0] != want[y0]).any() or (whole[y1 - 1] != want[y1 - 1]).any()      # the strip does not see across its edge
    # through the C entry: a plane pre-filled with a sentinel keeps the rows outside the strip
    winner, z, tri, color, mask = _painted(84, 100, 5)
    sentinel = np.full((84, 100, 3), -7.0, np.float32)
    for rows in ((37, 75), (0, 33), (83, 84)):
        got = _edge_aa(lib, winner, z, tri, E.P, color, edges=mask, y0=rows[0], y1=rows[1], out=sentinel)
        want = _model(winner, z, tri, E.P, color, edges=mask, y0=rows[0], y1=rows[1], out=sentinel)[0]
        assert (got[:rows[0]] == -7.0).all() and (got[rows[1]:] == -7.0).all()
        assert_bit_equal(got, want, f"rows {rows} into a sentinel")


def test_a_presorted_filler(oracle):
    """The corners are fetched through d_pos_of and the mask in the caller's order: a random mask tells a mix-up."""
    seed, T, H, W = 73, 3000, 256, 253
    s = _Scene(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), size_px=(3.0, 60.0)), H, W)
    f = filler(H, W, presort=True)
    mask = edge_mask("random", s.tri, seed)
    s.check(f, "presorted, all edges")
    assert f._order is not None
    s.check(f, "presorted, masked", edges=mask)
    perm = np.random.default_rng(1).permutation(T)
    assert (s.want(edges=mask[perm]) != s.want(edges=mask)).any()


# ---- 3. painted planes: what no rasterizer hands the pass -------------------------------------------------------------

@pytest.fixture(scope="module")
def edge(oracle):
    return E.scene()


def test_the_edge_scene(lib, edge):
    """tests/pass_edges.py's frame of 84 x 100: pixels far outside their winner (the clamp at 1/2), triangles of no area,
    NaN and infinite corners, a NaN z, winners beyond T; then d_pos_of with an entry beyond T."""
    s = edge
    for edges in (None, s.edges):
        want, a, direction = _model(s.winner, s.z, s.tri, E.P, s.color, edges=edges)
        assert_bit_equal(_edge_aa(lib, s.winner, s.z, s.tri, E.P, s.color, edges=edges), want, f"the edge scene, mask {edges is not None}")
        assert not np.isnan(want).any() and (a == np.float32(0.5)).sum() > 100 and (a > 0).sum() > 1000
    assert np.isnan(s.z).sum() > 100 and np.isnan(s.tri).any() and (s.winner >= s.T).any()
    want = _model(s.winner_without_gone, s.z, s.tri, E.P, s.color, edges=s.edges)[0]
    got = _edge_aa(lib, s.winner, s.z, s.moved, E.P, s.color, edges=s.edges, pos_of=s.pos_of)
    assert_bit_equal(got, want, "d_pos_of with an entry beyond T")
    assert_bit_equal(_model(s.winner, s.z, s.moved, E.P, s.color, edges=s.edges, pos_of=s.pos_of)[0], want, "the model's own d_pos_of")
    # T == 0 copies the rows, whatever the winners say
    got = _edge_aa(lib, s.winner, s.z, s.tri, E.P, s.color, T=0)
    assert_bit_equal(got, s.color, "T = 0")


def test_the_tie_of_the_depth_test(lib, oracle):
    """tests/pass_edges.py's tie scene — a near triangle A painted over a far one, B, that covers the frame, and A2, a
    copy of A with an edge of no length (0 / 0 in its barycentrics) — with depths of this pass's own: A's pixels at one
    depth, and B's pixels beside them, by the residue of x + 2 y, at exactly that depth (p is the near one from both
    sides), one ulp above it (A is the near one from both sides) or one below (B is, and A's pixel lies inside B: no
    edge)."""
    s = E.tie_scene()
    d = np.float32
    za = d(0.8125)
    z = s.z.copy()
    z[s.is_a | s.is_a2] = za
    beside = s.ring | s.ring2
    kind = (np.mgrid[0:s.H, 0:s.W][1] + 2 * np.mgrid[0:s.H, 0:s.W][0]) % 3
    z[beside] = np.where(kind == 0, za, np.where(kind == 1, np.nextafter(za, d(np.inf)), np.nextafter(za, d(-np.inf))))[beside]
    taken = {}
    for edges in (None, s.edges):
        want, a, direction = _model(s.winner, z, s.tri, E.P, s.color, edges=edges)
        assert_bit_equal(_edge_aa(lib, s.winner, z, s.tri, E.P, s.color, edges=edges), want, f"the tie scene, mask {edges is not None}")
        assert not np.isnan(want).any()
        taken[edges is None] = a > 0
    on = taken[True]
    assert (on & s.is_a).sum() > 10 and (on & s.ring).sum() >= 3 and 0 < taken[False].sum() < on.sum()
    # a B pixel beside A is blended only where it is the farther one (kind 1): at the tie and below, it asks its own triangle
    assert (kind[on & s.ring] == 1).all()
    # an A pixel all of whose differing neighbours are nearer is not blended
    flat = np.full_like(z, za)                                          # every depth equal: p is always the near one
    want, a, _ = _model(s.winner, flat, s.tri, E.P, s.color)
    assert_bit_equal(_edge_aa(lib, s.winner, flat, s.tri, E.P, s.color), want, "equal depths")
    assert not (a > 0)[s.winner == E.TIE_B].any() and (a > 0)[s.is_a].any()
    odd = np.where(s.is_a, d(np.nan), z).astype(d)
    want = _model(s.winner, odd, s.tri, E.P, s.color)[0]
    assert_bit_equal(_edge_aa(lib, s.winner, odd, s.tri, E.P, s.color), want, "NaN depths on the near triangle")


def test_lone_winners_on_the_seams_of_the_tiles(lib, oracle):
    """One covered pixel in a wavefront's two rows of 32, on every side of a tile seam: a wavefront that wrongly took the
    copy path, or a halo read from the wrong side, shows at that pixel and at its four neighbours."""
    frames = E.sparse_frames(1)
    assert len(frames) >= 2
    for k, s in enumerate(frames):
        want, a, _ = _model(s.winner, s.z, s.tri, E.P, s.color)
        for t, (x, y, _) in enumerate(s.lone):
            near = a[max(0, y - 1):y + 2, max(0, x - 1):x + 2]
            assert (near > 0).any(), (k, t, x, y)
        assert_bit_equal(_edge_aa(lib, s.winner, s.z, s.tri, E.P, s.color), want, f"sparse frame {k}")
        want = _model(s.winner, s.z, s.tri, E.P, s.color, edges=s.edges)[0]
        assert_bit_equal(_edge_aa(lib, s.winner, s.z, s.tri, E.P, s.color, edges=s.edges), want, f"sparse frame {k}, edge 0 alone")
    s = E.sparse_strip()
    y0, y1 = E.SPARSE_STRIP
    want, a, _ = _model(s.winner, s.z, s.tri, E.P, s.color, y0=y0, y1=y1)
    assert_bit_equal(_edge_aa(lib, s.winner, s.z, s.tri, E.P, s.color, y0=y0, y1=y1), want, "lone winners beside the strip")
    assert not a[y0].any() and not a[y1 - 1].any() and (a > 0).any()      # the winners just outside smooth nothing inside


# ---- 4. the host views and the Renderer ------------------------------------------------------------------------------

def test_the_views_stay_as_they_were_and_an_edit_is_smoothed(soup256):
    s = soup256
    f = filler(256, 256)
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    first = f.edge_aa()
    assert f._host_fresh and f.get_color_buffer() is view
    assert_bit_equal(view, s.cam.color_buffer, "the view after the pass: the plane was only read")
    assert_bit_equal(host(first), s.want(), "the result")
    view[:] = np.float32([10.0, 100.0, 200.0])
    view[100:140, 100:140] = np.float32([200.0, 10.0, 0.0])
    again = f.edge_aa()
    assert again.data_ptr() != first.data_ptr()
    flat = np.ascontiguousarray(view).copy()
    assert_bit_equal(host(again), s.want(base=flat), "over edited colours")
    assert_bit_equal(host(first), s.want(), "the first result is its own tensor")


WIRE = dict(width=2.0, color=LINE, feather=0.5)
AA = dict(contours=True, feature_angle=30)


def test_renderer_smooths_the_finished_frame(oracle):
    import torch
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    m, _ = textured_model()
    tri = m._vertices_by_triangles
    kw = dict(on_device=True, texture_pass={"perspective": True}, wireframe=WIRE)
    f, g = filler(256, 256), filler(256, 256)
    got = Renderer(f, GuroIllumination(GURO), antialias=AA, **kw).render(m)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.data_ptr() != f.color_buffer.data_ptr()
    base = host(Renderer(g, GuroIllumination(GURO), **kw).render(m)).copy()
    assert_bit_equal(host(f.get_color_tensor()), base, "the frame under the pass is the frame without it")
    cam = oracle.OracleFiller(256, 256, fov=45.0)
    view = contour_ref.contour_edges(tri, cam.proj_mat, 256, 256, edge_partners(tri), static=feature_edges(tri, 30.0), borders=True)[0]
    want, a, _ = edge_aa_ref.edge_aa(base, host(g.get_winner_tensor()), host(g.get_z_tensor()), tri, None, cam.proj_mat, edges=view)
    assert (a > 0).sum() > 500 and (want != base).any()
    assert_bit_equal(host(got), want, "Renderer(texture_pass, wireframe, antialias)")
    # (every edge of a soup is a border, so that view's mask is full; an explicit mask shows that the option reaches the pass)
    mask = edge_mask("random", tri)
    masked = edge_aa_ref.edge_aa(base, host(g.get_winner_tensor()), host(g.get_z_tensor()), tri, None, cam.proj_mat, edges=mask)[0]
    assert (masked != want).any()
    got = Renderer(f, GuroIllumination(GURO), antialias=dict(edges=mask), **kw).render(m)
    assert_bit_equal(host(got), masked, "Renderer(antialias={'edges': ...})")
    # None returns a fresh numpy array of the same bits
    again = Renderer(filler(256, 256), GuroIllumination(GURO), antialias=AA, **dict(kw, on_device=None)).render(m)
    assert isinstance(again, np.ndarray)
    assert_bit_equal(again, want, "on_device=None")
