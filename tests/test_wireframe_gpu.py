"""EdgeOnlyPixelBufferFiller.render_model on the GPU (csrc/wireframe.hip), bit for bit against the
reference's planes (tests/golden/wire_golden.json) and the host model of tests/wire_ref.py (itself
pinned on the reference's lines and the host loop in tests/test_wireframe_cpu.py)."""
import hashlib

import numpy as np
import pytest

from pass_scenes import wire_golden  # noqa: F401 (fixtures)
from util import assert_bit_equal, sha
from wire_ref import wire_plane

pytestmark = pytest.mark.gpu

LINE = (255.0, 64.5, 3.0)


def _filler(h, w, edges=True, forced=False, line=LINE):
    from cython3dmodelrenderer_amd.pixel_buffer_filler import EdgeOnlyPixelBufferFiller, LineBresenham
    return EdgeOnlyPixelBufferFiller(LineBresenham(), line, draw_edges=edges, force_triangle_colors=forced,
                                     h=h, w=w, device="cuda:0")


def _check_untouched(f, what):
    z, n = f.get_z_buffer(), f.get_normals_buffer()
    assert (z.view(np.uint32) == np.float32(1e6).view(np.uint32)).all(), what
    assert (n.view(np.uint32) == 0).all(), what


def _fitted(name, h=None, w=None):
    from cython3dmodelrenderer_amd import scenes
    fixture = {"cube256": "cube_inputs.npz", "trex1024": "trex_inputs.npz", "bunny1024": "bunny_inputs.npz"}[name]
    tri, col, _ = scenes.load_fixture(fixture)
    size = int(name[-4:]) if name[-4:].isdigit() else 256
    h, w = h or size, w or size
    has_col = name != "bunny1024"
    return scenes.fit_soup_to_frame(tri, h, w), (col if has_col else None), h, w


class _M:
    def __init__(self, tri, col):
        self._vertices_by_triangles, self._colors_by_triangles = tri, col


@pytest.mark.parametrize("name", ["cube256", "trex1024", "bunny1024"])
def test_golden_scenes_every_mode(name, wire_golden):
    entry = wire_golden["scenes"][name]
    tri, col, h, w = _fitted(name)
    assert hashlib.sha256(tri.tobytes()).hexdigest() == entry["vertices_sha"]
    for key, want in entry["planes"].items():
        edges, forced = key.startswith("edges"), key.endswith("forced")
        f = _filler(h, w, edges, forced, tuple(wire_golden["line_color"]))
        f.render_model(_M(tri, col))
        assert sha(f.get_color_buffer()) == want, (name, key)
        _check_untouched(f, (name, key))
        if forced:                              # the key plane is left zero for the next draw
            assert int(f._key.count_nonzero()) == 0


def _soup(rng, T, H, W, far=0.3, huge=0.1):
    """Triangles around an H x W frame: most near it, `far` of them up to 20 000 pixels off, `huge` of them
    anywhere in the domain (|c| < 2**30), a tenth degenerate."""
    tri = rng.uniform(-0.3, 1.3, (T, 3, 3)) * np.array([W, H, 1.0])
    u = rng.uniform(size=T)
    tri[u < far] = rng.uniform(-20000, 20000, (int((u < far).sum()), 3, 3))
    hv = u > 1 - huge
    tri[hv] = rng.uniform(-1.07e9, 1.07e9, (int(hv.sum()), 3, 3))
    deg = rng.uniform(size=T) < 0.1
    tri[deg, 2] = tri[deg, 0]
    tri = tri.astype(np.float32)
    col = rng.uniform(0, 255, (T, 3, 3)).astype(np.float32)
    return tri, col


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_soups_across_the_domain(seed):
    rng = np.random.default_rng(seed)
    H, W = [(200, 300), (256, 256), (97, 513)][seed - 1]
    tri, col = _soup(rng, 3000, H, W)
    for edges in (True, False):
        for forced in (False, True):
            f = _filler(H, W, edges, forced)
            f.render_arrays(tri, col)
            want = wire_plane(tri, H, W, LINE, edges, col if forced else None)
            assert_bit_equal(f.get_color_buffer(), want, (seed, edges, forced))
            _check_untouched(f, (seed, edges, forced))


def test_order_of_hundreds_of_triangles_through_one_pixel_and_two_ordered_draws():
    rng = np.random.default_rng(11)
    H, W = 64, 64
    T = 700
    tri = rng.uniform(-40, 100, (T, 3, 3)).astype(np.float32)
    tri[rng.integers(0, 3, T)[:, None] == np.arange(3)[None, :]] = np.float32(32.5)   # one vertex at (32, 32)
    col = rng.uniform(0, 255, (T, 3, 3)).astype(np.float32)
    for edges in (True, False):
        f = _filler(H, W, edges, True)
        f.render_arrays(tri, col)
        want = wire_plane(tri, H, W, LINE, edges, col)
        assert_bit_equal(f.get_color_buffer(), want, ("first", edges))
        # a second ordered draw on top: the key plane was reset by the first one
        tri2, col2 = tri[::-1].copy(), rng.uniform(0, 255, (T, 3, 3)).astype(np.float32)
        f.render_arrays(tri2, col2)
        want = wire_plane(tri2, H, W, LINE, edges, col2, base=want)
        assert_bit_equal(f.get_color_buffer(), want, ("second", edges))
        assert int(f._key.count_nonzero()) == 0


def test_compositing_onto_prior_content_and_host_edits():
    rng = np.random.default_rng(5)
    H, W = 120, 90
    tri, col = _soup(rng, 400, H, W, far=0.1, huge=0.0)
    f = _filler(H, W, True, True)
    f.render_arrays(tri[:200], col[:200])
    view = f.get_color_buffer()
    want = wire_plane(tri[:200], H, W, LINE, True, col[:200])
    assert_bit_equal(view, want, "first")
    view[10:40, 5:60] = 7.25                   # an in-place edit of the handed-out view
    f.get_z_buffer()[0, 0] = 3.0
    want = wire_plane(tri[200:], H, W, LINE, True, col[200:], base=view.copy())
    f.render_arrays(tri[200:], col[200:])
    assert_bit_equal(view, want, "composited on the edit")       # the same array shows the new draw
    assert f.get_z_buffer()[0, 0] == 3.0
    t = f.get_color_tensor().cpu().numpy()
    assert_bit_equal(t, want, "tensor")
    u8 = f.present_u8().cpu().numpy()
    assert np.array_equal(u8, want[::-1].astype(np.uint8))
    f.clear()
    assert (f.get_color_buffer() == 0).all() and (f.get_z_buffer() == np.float32(1e6)).all()
    # clear=True draws on the initial state
    f.get_color_buffer()[:] = 9.0
    f.render_arrays(tri, col, clear=True)
    assert_bit_equal(f.get_color_buffer(), wire_plane(tri, H, W, LINE, True, col), "clear=True")
    _check_untouched(f, "clear=True")


def test_model_device_model_and_torch_inputs():
    import torch
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    tri, col, h, w = _fitted("trex1024", 512, 384)
    T = tri.shape[0]
    corners = tri.reshape(-1, 3)
    faces = np.arange(3 * T, dtype=np.int32).reshape(T, 3)
    m = Model(corners, faces, normals=np.zeros_like(corners), triangles_normals=faces, recalculate_normals=False)
    m._colors_by_triangles = col
    for forced in (False, True):
        want = wire_plane(tri, h, w, LINE, True, col if forced else None)
        for src in (m, DeviceModel(m), _M(torch.from_numpy(tri).cuda(), torch.from_numpy(col).cuda()),
                    _M(torch.from_numpy(tri), torch.from_numpy(col).double())):
            f = _filler(h, w, True, forced)
            f.render_model(src)
            assert_bit_equal(f.get_color_buffer(), want, (type(src).__name__, forced))


@pytest.mark.parametrize("illum", ["none", "guro"])
def test_renderer_with_every_on_device(illum):
    import torch
    from cython3dmodelrenderer_amd import Renderer
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, NoIllumination
    tri, col, h, w = _fitted("cube256")
    model = _M(tri, col)
    for forced in (False, True):
        plane = wire_plane(tri, h, w, LINE, True, col if forced else None)
        want = plane.copy()
        if illum == "guro":
            GuroIllumination((0.3, -0.2, 1.0)).draw_illumination(want, np.zeros_like(want))
        results = {}
        for on_device in (None, False, True, "fused"):
            ill = NoIllumination() if illum == "none" else GuroIllumination((0.3, -0.2, 1.0))
            r = Renderer(_filler(h, w, True, forced), ill, image_height=h, image_width=w, use_tqdm=False,
                         on_device=on_device)
            out = r.render(model)
            out = out.cpu().numpy() if isinstance(out, torch.Tensor) else np.array(out)
            assert_bit_equal(out, want, (illum, forced, on_device))
            results[on_device] = out
        assert np.array_equal(results["fused"].view(np.uint32), results[True].view(np.uint32))
        if illum == "none":
            assert (want != 0).any()


def test_out_of_domain_raises_before_drawing():
    rng = np.random.default_rng(3)
    H, W = 64, 80
    tri, col = _soup(rng, 50, H, W, far=0.0, huge=0.0)
    for forced in (False, True):
        f = _filler(H, W, True, forced)
        f.render_arrays(tri, col)
        before = f.get_color_buffer().copy()
        for bad in (np.nan, np.inf, -np.inf, 2.0 ** 30, -(2.0 ** 30)):
            for axis in (0, 1):
                t = tri.copy()
                t[37, 2, axis] = bad
                for clear in (False, True):
                    with pytest.raises(ValueError):
                        f.render_arrays(t, col, clear=clear)
                    assert_bit_equal(f.get_color_buffer(), before, (forced, bad, axis, clear))
                    _check_untouched(f, (forced, bad, axis, clear))
        if forced:
            assert int(f._key.count_nonzero()) == 0
        # z is not checked: a NaN or a huge z draws as the reference does
        t = tri.copy()
        t[:, :, 2] = np.nan
        f.render_arrays(t, col)
        assert_bit_equal(f.get_color_buffer(), wire_plane(tri, H, W, LINE, True, col if forced else None, base=before),
                         ("z", forced))
    f = _filler(H, W, True, True)
    with pytest.raises(ValueError):
        f.render_model(_M(tri, None))


def test_trex_8192_large_frame_long_edges():
    tri, col, h, w = _fitted("trex1024", 8192, 8192)
    for edges, forced in ((True, False), (True, True), (False, True)):
        f = _filler(h, w, edges, forced)
        f.render_arrays(tri, col)
        got = f.get_color_tensor().cpu().numpy()
        assert_bit_equal(got, wire_plane(tri, h, w, LINE, edges, col if forced else None), (edges, forced))
