"""The hidden lines on the GPU (csrc/wireframe.hip's k_wire_hidden through AdvancedPixelBufferFiller.hidden_line_pass, the
C entry and Renderer(wireframe={"hidden": ...})), bit for bit against the host model of tests/hidden_ref.py evaluated on
the oracle's frames and on painted planes (itself pinned in tests/test_hidden_cpu.py).  Every case also checks that the
key plane is zero again after the call and that z, normals and the winner plane were only read."""
import ctypes as C

import numpy as np
import pytest

import contour_ref
import hidden_ref
import outline_ref
import pass_edges as E
import ssaa_ref
from pass_scenes import Scene, TriangleModel, edge_mask, filler, host, lib, soup_fixture, trex_arrays, trex_fixture  # noqa: F401
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)              # what GuroIllumination is constructed with
LINE = (250.0, 240.0, 20.0)


class _Scene(Scene):
    def want(self, base=None, **kw):
        """(the model's colours over `base` — the oracle's if None —, its classes)."""
        kw = dict(kw)
        kw["line"] = kw.pop("color", kw.pop("line", (0, 0, 0)))
        return hidden_ref.hidden_lines(self.cam.color_buffer if base is None else base, self.cam.winner, self.cam.z_buffer,
                                       self.tri, None, self.cam.proj_mat, **kw)

    def check(self, f, what, model_edges=None, rows=None, **kw):
        """Draw, run the pass with `kw` and compare with the model (under `model_edges` for a mask made on the device)."""
        self.draw(f)
        assert f.hidden_line_pass(**kw) is None
        if model_edges is not None:
            kw = dict(kw, edges=model_edges)
        y0, y1 = (0, self.H) if rows is None else rows
        want, key = self.want(y0=y0, y1=y1, **kw)
        assert_bit_equal(host(f.get_color_tensor())[y0:y1], want[y0:y1], f"{what}: the colours")
        assert tuple(f._hidden_key.shape) == (self.H, self.W) and not host(f._hidden_key).any(), f"{what}: the key plane is zero again"
        self.check_planes(f, what)
        return want, key


trex256 = trex_fixture(_Scene)
soup256 = soup_fixture(_Scene)


# ---- 1. T-Rex and the soup at 256 x 256 ------------------------------------------------------------------------------

def test_trex_every_mask_rule_and_bias(trex256):
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    s = trex256
    f = filler(256, 256)
    static = feature_edges(s.tri, 30.0)
    partners = edge_partners(s.tri)
    view = contour_ref.contour_edges(s.tri, s.cam.proj_mat, 256, 256, partners, static=static, borders=True)[0]
    hidden = {}
    for name, edges in (("all", None), ("feature", static), ("contours", "device")):
        for rule in (True, False):
            for bias in (0.0, 1e-3):
                what = f"T-Rex, {name} edges, rule {rule}, bias {bias}"
                kw = dict(color=LINE, opacity=0.75, dash=(3, 2), use_winner=rule, depth_bias=bias)
                if name == "contours":
                    # the mask of the view, classified on the device and handed over as the device tensor it is
                    s.draw(f)
                    mask = f.contour_edges(partners, static=static, borders=True)
                    assert np.array_equal(host(mask), view)
                    want, key = s.check(f, what, model_edges=view, edges=mask, **kw)
                else:
                    want, key = s.check(f, what, edges=edges, **kw)
                hidden[name, rule, bias] = int((key == 1).sum())
                assert hidden[name, rule, bias] > 0 and (want != s.cam.color_buffer).any(), what
    print(hidden)
    for name in ("all", "feature", "contours"):
        for bias in (0.0, 1e-3):
            assert hidden[name, True, bias] <= hidden[name, False, bias]
        assert hidden[name, True, 0.0] < hidden[name, False, 0.0]      # at bias 0 the rule takes back the edges IN the surface
    # the defaults
    s.check(f, "T-Rex, the defaults")


def test_the_soup_needs_many_workgroups_and_a_second_trip(soup256):
    s = soup256
    S = hidden_ref.segments(s.tri, s.cam.proj_mat, 256, 256)
    n = hidden_ref.steps(S, 256, 256)[0]
    per_group = np.bincount((3 * S["i"] + S["e"])[n] // 256)
    assert len(per_group) >= 30 and per_group.max() > 2 * 256, (len(per_group), per_group.max())
    f = filler(256, 256)
    for kw in (dict(color=LINE), dict(color=LINE, edges=edge_mask("random", s.tri), dash=(1, 1), use_winner=False, opacity=1.0),
               dict(dash=(5, 0), depth_bias=0.0)):
        want, key = s.check(f, f"the soup, {sorted(kw)}", **kw)
        assert (key == 1).sum() > 500 and (key == 2).sum() > 500


def test_a_presorted_filler(oracle):
    """The corners are fetched through d_pos_of; the mask and the winner rule are in the caller's order: a random mask
    tells a mix-up."""
    seed, T, H, W = 73, 3000, 256, 253
    s = _Scene(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), size_px=(3.0, 60.0)), H, W)
    f = filler(H, W, presort=True)
    mask = edge_mask("random", s.tri, seed)
    s.check(f, "presorted, all edges", color=LINE)
    assert f._order is not None
    want, _ = s.check(f, "presorted, masked", color=LINE, edges=mask)
    perm = np.random.default_rng(1).permutation(T)
    assert (s.want(color=LINE, edges=mask[perm])[0] != want).any()


def test_a_row_strip_whose_ends_are_no_multiples_of_eight(oracle):
    y0, y1 = 37, 139
    s = _Scene(oracle, trex_arrays(), 200, 173, y0=y0, y1=y1)
    f = filler(200, 173, row_strip=(y0, y1))
    s.draw(f)
    f.synchronize()
    # rows outside the strip: colours that must keep their bits, and depths that WOULD hide every edge there
    f.color_buffer[:y0] = 7.5
    f.color_buffer[y1:] = -2.25
    f.z_buffer[:y0] = -5.0
    f.z_buffer[y1:] = -5.0
    f.hidden_line_pass(color=LINE, dash=(2, 1))
    got = host(f.get_color_tensor())
    assert (got[:y0] == 7.5).all() and (got[y1:] == -2.25).all()
    want, key = s.want(color=LINE, dash=(2, 1), y0=y0, y1=y1)
    assert (key == 1).sum() > 300 and not key[:y0].any() and not key[y1:].any()
    assert_bit_equal(got[y0:y1], want[y0:y1], "the strip's rows")
    assert not host(f._hidden_key).any()


# ---- 2. through the C entry: painted planes, odd segments -------------------------------------------------------------

def _hidden(lib, winner, z, tri, P, color, edges=None, T=None, pos_of=None, y0=0, y1=None, line=LINE, opacity=0.5, dash=(4, 4),
            depth_bias=1e-3, use_winner=True):
    """crender_wire_hidden on numpy planes: the colour plane afterwards.  The key plane is zero again and everything else
    was only read."""
    import torch
    from cython3dmodelrenderer_amd import _capi
    H, W = winner.shape
    T = tri.shape[0] if T is None else T
    y1 = H if y1 is None else y1
    pos_of = None if pos_of is None else np.ascontiguousarray(pos_of).view(np.int32)      # (the same 32 bits)
    given = (winner, z, tri if len(tri) else None, pos_of, edges)
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in given]
    d_color = torch.from_numpy(np.ascontiguousarray(color)).cuda()
    d_key = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = [None if a is None else a.data_ptr() for a in dev]
    _capi.check(lib.crender_wire_hidden(ptr[0], ptr[1], ptr[2] if T else None, T, ptr[3], _capi.f32_16(P), ptr[4],
                                        (C.c_float * 3)(*line), opacity, dash[0], dash[1], depth_bias, d_key.data_ptr(),
                                        d_color.data_ptr(), H, W, y0, y1, _capi.WIRE_HIDDEN_USE_WINNER if use_winner else 0, st),
                "crender_wire_hidden")
    got = host(d_color)
    assert not host(d_key).any(), "the key plane is zero again"
    for a, b, name in zip(dev, given, ("winner", "z", "tri", "pos_of", "edges")):
        if a is not None:
            assert_bit_equal(host(a), np.ascontiguousarray(b), f"{name} is only read")
    return got


def _model(winner, z, tri, P, color, edges=None, pos_of=None, **kw):
    return hidden_ref.hidden_lines(color, winner, z, tri, pos_of, P, edges=edges, **dict(dict(line=LINE), **kw))


DEPTHS = np.float32([0.5, 0.7, 0.75, 0.8, 0.9, 0.95, 1e6])


def _painted(H, W, seed, T=40):
    """Planes no rasterizer makes, for a frame of any shape: triangles across the frame and beyond it, a winner plane of
    random indices with background and winners beyond T among them, depths around the triangles' own, random colours."""
    rng = np.random.default_rng(seed)
    sx = rng.uniform(-12, W + 12, (T, 3))
    sy = rng.uniform(-12, H + 12, (T, 3))
    tri = np.ascontiguousarray(E.unproject(sx, sy, rng.uniform(0.6, 2.5, (T, 3)), W, H))
    winner = rng.integers(-1, T + 2, (H, W)).astype(np.int32)
    z = rng.choice(DEPTHS, (H, W))
    color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    mask = rng.integers(0, 256, T).astype(np.uint8)
    return winner, z, tri, color, mask


@pytest.mark.parametrize("H,W", [(1, 1), (33, 7), (7, 33)])
def test_frames_of_one_pixel_and_of_odd_sizes(lib, oracle, H, W):
    winner, z, tri, color, mask = _painted(H, W, 1000 * H + W)
    seen = 0
    for kw in (dict(), dict(edges=mask, dash=(2, 1)), dict(use_winner=False, dash=(1, 0), depth_bias=0.0, opacity=1.0)):
        want, key = _model(winner, z, tri, E.P, color, **kw)
        assert_bit_equal(_hidden(lib, winner, z, tri, E.P, color, **kw), want, f"{H} x {W}, painted, {sorted(kw)}")
        seen += int((key == 1).sum())
    assert seen >= (0 if H * W == 1 else 20)
    if H * W == 1:
        # one pixel, one segment through it, behind what the pixel shows: the pixel is the line's
        one = np.ascontiguousarray(E.unproject(np.float64([[-3, 4, 0]]), np.float64([[-2, 3, 9]]), 2.0, 1, 1))
        z1, w1, c1 = np.float32([[0.5]]), np.int32([[-1]]), np.float32([[[10.0, 20.0, 30.0]]])
        want, key = _model(w1, z1, one, E.P, c1, dash=(1, 0), opacity=1.0)
        assert key[0, 0] == 1 and (want[0, 0] == np.float32(LINE)).all()
        assert_bit_equal(_hidden(lib, w1, z1, one, E.P, c1, dash=(1, 0), opacity=1.0), want, "1 x 1, one line")


def test_segments_that_are_skipped_or_clipped(lib, oracle):
    """tests/hidden_ref.py's hand-built set on a 64 x 64 frame — lines through each of the four sides, of length 0, of half
    a billion steps, corners that are NaN, infinite, at or beyond 2^30, at z <= 0 — behind a first workgroup of 256 segments
    that are ALL skipped (86 triangles behind the camera), and with an order that sends some triangles beyond T."""
    odd, walked = hidden_ref.odd_segments()
    behind = np.ascontiguousarray(E.unproject(np.full((86, 3), 30.0), np.full((86, 3), 30.0), 1.0, 64, 64))
    behind[:, :, 2] = np.float32([-1.0, 0.0, np.nan])[None, :]
    tri = np.ascontiguousarray(np.concatenate([behind, odd]))
    T = len(tri)
    S = hidden_ref.segments(tri, E.P, 64, 64)
    assert sorted(zip((S["i"] - 86).tolist(), S["e"].tolist())) == walked and (3 * S["i"] + S["e"]).min() >= 256
    rng = np.random.default_rng(7)
    winner = rng.integers(-1, T + 2, (64, 64)).astype(np.int32)
    z = rng.choice(DEPTHS, (64, 64))
    color = rng.uniform(0, 255, (64, 64, 3)).astype(np.float32)
    mask = rng.integers(0, 256, T).astype(np.uint8)
    for kw in (dict(dash=(1, 0)), dict(dash=(3, 3), use_winner=False), dict(edges=mask, depth_bias=0.0)):
        want, key = _model(winner, z, tri, E.P, color, **kw)
        assert (key == 1).sum() > 30 and (key == 2).sum() > 30
        assert_bit_equal(_hidden(lib, winner, z, tri, E.P, color, **kw), want, f"the odd segments, {sorted(kw)}")
    # d_pos_of: the triangles moved, some sent beyond T
    perm = rng.permutation(T).astype(np.uint32)
    moved = np.empty_like(tri)
    moved[perm] = tri
    gone = np.arange(T) % 5 == 3
    perm[gone] = np.uint32([T, T + 7, 2 ** 32 - 1] * T)[:int(gone.sum())]
    want, key = _model(winner, z, moved, E.P, color, edges=mask, pos_of=perm)
    kept = tri.copy()
    kept[gone, :, 2] = -1.0                                             # (the same as a triangle that is skipped)
    assert_bit_equal(want, _model(winner, z, kept, E.P, color, edges=mask)[0], "the model's own d_pos_of")
    assert_bit_equal(_hidden(lib, winner, z, moved, E.P, color, edges=mask, pos_of=perm), want, "d_pos_of with entries beyond T")


def test_a_z_plane_of_nan_and_infinities_and_no_triangles(lib, oracle):
    winner, z, tri, color, mask = _painted(84, 100, 5)
    rng = np.random.default_rng(6)
    odd = rng.choice(np.float32([np.nan, np.inf, -np.inf, 0.5, 1e6, -0.0]), z.shape)
    for kw in (dict(dash=(1, 0)), dict(edges=mask, use_winner=False)):
        want, key = _model(winner, odd, tri, E.P, color, **kw)
        assert (key == 1).sum() > 100 and (key == 2).sum() > 100 and not np.isnan(want).any()
        assert_bit_equal(_hidden(lib, winner, odd, tri, E.P, color, **kw), want, f"NaN and infinite depths, {sorted(kw)}")
        assert not (key[np.isnan(odd) | (odd == np.inf) | (odd == np.float32(1e6))] == 1).any()      # they never hide
    # T == 0 returns without a launch, whatever the planes hold
    assert_bit_equal(_hidden(lib, winner, odd, tri, E.P, color, T=0), color, "T = 0 with a d_tri")
    assert_bit_equal(_hidden(lib, winner, odd, tri[:0], E.P, color), color, "T = 0")
    # rows through the C entry: a strip of one row, and the last rows
    for rows in ((37, 38), (75, 84)):
        want = _model(winner, z, tri, E.P, color, edges=mask, y0=rows[0], y1=rows[1])[0]
        assert (want[rows[0]:rows[1]] != color[rows[0]:rows[1]]).any()
        assert_bit_equal(_hidden(lib, winner, z, tri, E.P, color, edges=mask, y0=rows[0], y1=rows[1]), want, f"rows {rows}")


# ---- 3. the host views and the Renderer ------------------------------------------------------------------------------

def test_an_edit_made_in_a_view_is_drawn_over_and_the_view_shows_the_lines(soup256):
    s = soup256
    f = filler(256, 256)
    s.draw(f)
    view = f.get_color_buffer()
    assert_bit_equal(view, s.cam.color_buffer, "before the pass")
    view[100:140, 100:140] = np.float32([200.0, 10.0, 0.0])
    edited = np.ascontiguousarray(view).copy()
    f.hidden_line_pass(color=LINE)
    key = f._hidden_key
    assert f.get_color_buffer() is view
    want, _ = s.want(base=edited, color=LINE)
    assert_bit_equal(view, want, "the view after the pass, over the edit")
    f.hidden_line_pass(color=LINE, dash=(1, 0))
    assert f._hidden_key is key and not host(key).any()                  # the plane is kept, and zero again


FILL = (255.0, 255.0, 255.0)
H, W = 96, 160


def test_one_session_through_the_renderer(oracle):
    """fill, outline, the contours of the view and the hidden lines together, as a drawing of a body: the Renderer's
    frame against the chained host models (the light, the outline, the hidden lines), then the same supersampled."""
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    tri = contour_ref.place(contour_ref.open_cylinder(), (25, 40, 10))
    s = _Scene(oracle, (tri,) + contour_ref.attributes(tri), H, W)
    assert s.covered > 3000
    model = TriangleModel(s.tri, s.col, s.nrm)
    guro = GuroIllumination(GURO)
    opts = dict(outline=True, fill=FILL, color=(0.0, 0.0, 0.0), feature_angle=15.0, contours=True,
                hidden=dict(color=(90.0, 90.0, 90.0), opacity=1.0, dash=(3, 2)))
    lit = ssaa_ref.shade(s.cam.color_buffer, s.cam.normals_buffer, GURO)
    mask = contour_ref.contour_edges(tri, s.cam.proj_mat, W, H, edge_partners(tri), static=feature_edges(tri, 15.0), borders=True)[0]
    lines = outline_ref.wire_pass(lit, s.cam.winner, s.cam.z_buffer, tri, s.cam.proj_mat, line=(0.0, 0.0, 0.0), fill=FILL, edges=mask)
    want, key = s.want(base=lines, color=(90.0, 90.0, 90.0), opacity=1.0, dash=(3, 2), edges=mask)
    assert (key == 1).sum() > 50 and (want != lines).any()               # the far side of the tube, dashed
    assert (want[key == 1] == np.float32(90.0)).all()                    # drawn AFTER the fill, not under it
    f = filler(H, W)
    got = Renderer(f, guro, on_device=True, wireframe=opts).render(model)
    assert_bit_equal(host(got), want, "Renderer(wireframe={fill, outline, contours, hidden})")
    s.check_planes(f, "the Renderer's frame")
    assert not host(f._hidden_key).any()
    again = Renderer(f, guro, on_device=None, wireframe=opts).render(model)
    assert isinstance(again, np.ndarray)
    assert_bit_equal(again, want, "on_device=None: the numpy view")
    # hidden=True: the defaults, with the mask of the wire pass
    plain = host(Renderer(f, guro, on_device=True, wireframe=dict(opts, hidden=True)).render(model))
    assert_bit_equal(plain, s.want(base=lines, edges=mask)[0], "hidden=True")
    # supersampled: the filler is the large frame; the passes run on it, then the resolve
    f = filler(H, W)
    small = Renderer(f, guro, None, H // 2, W // 2, on_device=True, supersample=2, wireframe=opts).render(model)
    assert_bit_equal(host(f.get_color_tensor()), want, "supersample=2: the supersampled frame")
    assert_bit_equal(host(small), ssaa_ref.resolve(want, 2), "supersample=2: the resolved image")
