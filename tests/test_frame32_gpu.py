"""The swap chain's frame kernel for small scenes on 32-pixel tiles (include/crender_frame32.h, csrc/frame32.hip):
the same planes, bit for bit (compared as uint32), as the oracle and as the same frames through the general frame
kernel (crender_pipeline_submit), on the same kind of plans; ``crender_plan_debug_check`` on every plan after the
frames; and ``crender_frame32_last`` asserted, so that no case passes by delegating.

Everything runs on a small harness over the C ABI (two plans per slot, look-ahead on, no winner plane unless a case
asks for one): frames are at most 100 x 80 pixels with a few hundred triangles, a case is some dozens of launches of
microseconds each.  Every scene keeps more than four triangles per tile: below that a plan without a record yet
picks the pixel owners' kernel, and the frame would be the general code's."""
import ctypes as C

import numpy as np
import pytest

from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

FOV = 45.0
LIGHT = (0.3, -0.5, 0.8)


def _capi():
    from cython3dmodelrenderer_amd import _capi
    return _capi


def _device(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays]


class Chain:
    """A look-ahead pipeline of `depth` slots over 32-pixel plans, its framebuffer sets pre-filled with junk (a frame
    must wipe what the caller wrote), driven through crender_frame32_submit (`frame32`) or crender_pipeline_submit."""

    def __init__(self, h, w, max_T, depth, frame32, winner=False):
        import torch
        from cython3dmodelrenderer_amd import lowlevel as L
        capi = _capi()
        self.lib, self.capi, self.h, self.w, self.depth, self.frame32 = capi.load(), capi, h, w, depth, frame32
        self.plans = [L.Plan(h, w, max_T, tile=32) for _ in range(2 * depth)]
        self.fbs = [L.FrameBuffers(h, w, winner=winner) for _ in range(depth)]
        for fb in self.fbs:
            fb.z.fill_(7.0); fb.color.fill_(7.0); fb.normals.fill_(7.0)
        self.P = capi.f32_16(L.projection_matrix(FOV, 0.1, 1000.0, h, w))
        self.stream = torch.cuda.current_stream().cuda_stream
        self.pipe = C.c_void_p()
        arr = lambda ps: (C.c_void_p * depth)(*[p.handle.value for p in ps])
        capi.check(self.lib.crender_pipeline_create(C.byref(self.pipe), arr(self.plans[:depth]), depth), "create")
        capi.check(self.lib.crender_pipeline_set_lookahead(self.pipe, arr(self.plans[depth:]), depth), "lookahead")
        self.inputs = None

    def bind(self, inputs, slots=None, flags=None, winner=False):
        capi = self.capi
        flags = capi.FUSED_CLEAR | capi.OVERLAPPED_FRAMES if flags is None else flags
        self.inputs = inputs                     # (kept alive)
        t, c, n = inputs
        for k in (range(self.depth) if slots is None else slots):
            fb = self.fbs[k]
            capi.check(self.lib.crender_pipeline_bind(
                self.pipe, k, t.data_ptr(), c.data_ptr(), n.data_ptr(), t.shape[0], self.P, fb.z.data_ptr(),
                fb.color.data_ptr(), fb.normals.data_ptr(), fb.winner.data_ptr() if winner else None, flags), "bind")

    def submit(self, expect=None):
        fn = self.lib.crender_frame32_submit if self.frame32 else self.lib.crender_pipeline_submit
        self.capi.check(fn(self.pipe, self.stream), "submit")
        if self.frame32 and expect is not None:
            assert self.lib.crender_frame32_last(self.pipe) == int(expect), "the frame took the other kernel"

    def join(self, check=True):
        import torch
        self.capi.check(self.lib.crender_pipeline_join(self.pipe, self.stream), "join")
        torch.cuda.synchronize()
        if check:
            for plan in self.plans:
                plan.debug_check()

    def frame(self, expect=None):
        """One frame, joined, every plan checked."""
        self.submit(expect)
        self.join()

    def planes(self, k, winner=False):
        fb = self.fbs[k]
        out = [fb.z.cpu().numpy(), fb.color.cpu().numpy(), fb.normals.cpu().numpy()]
        return out + [fb.winner.cpu().numpy()] if winner else out

    def close(self):
        import torch
        torch.cuda.synchronize()
        if self.pipe:
            self.lib.crender_pipeline_destroy(self.pipe)
            self.pipe = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _want(oracle, scene, h, w):
    ref = oracle.OracleFiller(h, w, fov=FOV)
    ref.render_arrays(*scene)
    return [ref.z_buffer.copy(), ref.color_buffer.copy(), ref.normals_buffer.copy()]


def _same(got, want, what):
    for g, w_, name in zip(got, want, ("z", "colour", "normal", "winner")):
        assert_bit_equal(g, w_, f"{what}: {name}")


def _soup(seed, T, w, size=(2, 30), **kw):
    return random_soup(np.random.default_rng(seed), T, w, size_px=size, **kw)


def _boxes(oracle, tri, h, w):
    """Pixel boxes [xl, xr) x [yt, yb) of the projected triangles (.pyx:132-175)."""
    proj = oracle.project(tri, oracle.projection_matrix(FOV, 0.1, 1000.0, h, w), w, h)
    x, y = proj[:, :, 0], proj[:, :, 1]
    cl = lambda v, hi: np.clip(np.ceil(v), 0, hi).astype(np.int64)
    return (cl(np.minimum(x.min(1), w), w), cl(np.maximum(x.max(1), 0), w),
            cl(np.minimum(y.min(1), h), h), cl(np.maximum(y.max(1), 0), h))


def _inside(oracle, scene, h, w, x0, y0, x1, y1):
    """The scene's triangles (all front-facing) whose non-empty box lies inside [x0, x1) x [y0, y1)."""
    xl, xr, yt, yb = _boxes(oracle, scene[0], h, w)
    keep = (xl < xr) & (yt < yb) & (xl >= x0) & (xr <= x1) & (yt >= y0) & (yb <= y1)
    return [a[keep] for a in scene]


def _tile_scene(oracle, n, h=64, w=64, seed=5):
    """Exactly `n` records in tile (1, 1) — every one of them wholly inside it — and 40 in tile (0, 0)."""
    cand = _soup(seed, 20000, w, size=(2, 7), frac_backface=0.0, margin=0.0)
    target = _inside(oracle, cand, h, w, 33, 33, 63, 63)
    pad = _inside(oracle, cand, h, w, 1, 1, 31, 31)
    assert len(target[0]) >= n and len(pad[0]) >= 40
    # (the pad first: the target's indices, and so its depth ties, sit at the high end)
    return [np.concatenate([p[:40], t[:n]]) for p, t in zip(pad, target)]


def _pair(h, w, max_T, depth, **kw):
    return Chain(h, w, max_T, depth, True, **kw), Chain(h, w, max_T, depth, False, **kw)


def _rounds(chain, rounds, expect=True):
    """`rounds` times: one frame per slot, then a join and the check of every plan (a join restarts the chain at
    slot 0); then one more frame, joined and checked alone."""
    for _ in range(rounds):
        for _ in range(chain.depth):
            chain.submit(expect)
        chain.join()
    chain.frame(expect)


def _run_both(oracle, scene, h, w, depth, rounds, static=True, what=""):
    """One scene on both chains (_rounds); every set against the oracle and against the general kernel's."""
    capi = _capi()
    want = _want(oracle, scene, h, w)
    dev = _device(scene)
    new, old = _pair(h, w, len(scene[0]), depth)
    flags = capi.FUSED_CLEAR | capi.OVERLAPPED_FRAMES | (capi.STATIC_INPUTS if static else 0)
    for chain in (new, old):
        chain.bind(dev, flags=flags)
        _rounds(chain, rounds)
    for k in range(depth):
        _same(new.planes(k), want, f"{what} set {k} against the oracle")
        _same(new.planes(k), old.planes(k), f"{what} set {k} against the general kernel")
    new.close(); old.close()


@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("hw", [(64, 64), (80, 96), (72, 100), (72, 98)])
def test_frames_in_flight_are_exact(oracle, hw, depth):
    """A burst that comes round to every slot twice and once more, nothing joined in between: the binning
    wavefronts of one launch fill the bins the slot's next launch reads.  80 rows end in a partial tile row,
    100 and 98 columns in a partial tile column (98: no 16-byte rows either)."""
    h, w = hw
    scene = _soup(11, 300, w)
    want = _want(oracle, scene, h, w)
    dev = _device(scene)
    new, old = _pair(h, w, 300, depth)
    for chain in (new, old):
        chain.bind(dev)
        for _ in range(2 * depth + 1):
            chain.submit(expect=True)
        chain.join()
    for k in range(depth):
        _same(new.planes(k), want, f"{h}x{w} depth {depth} set {k} against the oracle")
        _same(new.planes(k), old.planes(k), f"{h}x{w} depth {depth} set {k} against the general kernel")
    new.close(); old.close()


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513])
def test_list_lengths(oracle, n):
    """A tile's list of n records: the split thresholds (32, 64), the batch boundary (256), and with 513 winners in
    batches other than the last.  Five frames of a depth-2 chain whose look-ahead survives the joins
    (CRENDER_STATIC_INPUTS): from the third on they render from bins the kernel's own binning wavefronts filled."""
    scene = _tile_scene(oracle, n)
    assert len(scene[0]) == 40 + n
    _run_both(oracle, scene, 64, 64, 2, 2, what=f"{n} records")


def test_a_large_record_among_small_ones(oracle):
    h, w = 80, 96
    small = _soup(21, 400, w, size=(2, 10))
    big = np.array([[[-40.0, -40.0, 20.0], [40.0, -40.0, 20.0], [0.0, 60.0, 20.0]]], np.float32)   # covers the frame, behind
    scene = [np.concatenate([small[0][:200], big, small[0][200:]]),
             np.concatenate([small[1][:200], np.full((1, 3, 3), 99.0, np.float32), small[1][200:]]),
             np.concatenate([small[2][:200], np.array([[[0.1, 0.2, -1.0]] * 3], np.float32), small[2][200:]])]
    want = _want(oracle, scene, h, w)
    assert (want[0] < 1e6).all()                # the large triangle does cover every pixel
    _run_both(oracle, scene, h, w, 2, 2, what="large among small")


@pytest.mark.parametrize("copies", [2, 3])
def test_exact_depth_ties(oracle, copies):
    """Coplanar copies of a triangle at different indices, with other colours: the highest index wins every pixel
    (its index is in the compared bits of the slotted keys)."""
    h, w = 64, 64
    base = _tile_scene(oracle, 100)
    rng = np.random.default_rng(3)
    scene = [a.copy() for a in base]
    for src, others in ((100, [60, 130]), (5, [30, 2])):      # a triangle of the target tile, one of the pad
        for dst in others[:copies - 1]:
            scene[0][dst] = base[0][src]
            scene[2][dst] = base[2][src]
            scene[1][dst] = rng.uniform(0, 255, (3, 3)).astype(np.float32)
    _run_both(oracle, scene, h, w, 2, 2, what=f"{copies} coplanar copies")


def test_degenerate_and_stale_input(oracle):
    """NaN depths and zero-area triangles among ordinary ones; then, on the same plans, a scene of far fewer
    triangles: the slabs keep the first scene's entries, whose indices lie beyond the new triangle count."""
    h, w = 80, 96
    scene = _soup(31, 300, w, size=(2, 20))
    scene[0][10, :, 2] = np.nan                               # NaN z at every vertex
    scene[0][11, 1, 2] = np.nan                               # ... at one
    scene[0][12, 1] = scene[0][12, 0]                         # two equal vertices
    scene[0][13, 1] = scene[0][13, 2] = scene[0][13, 0]       # a point
    scene[0][14, 2] = (scene[0][14, 0] + scene[0][14, 1]) / 2  # collinear
    few = [a[200:260].copy() for a in _soup(32, 300, w, size=(2, 20))]
    capi = _capi()
    flags = capi.FUSED_CLEAR | capi.OVERLAPPED_FRAMES | capi.STATIC_INPUTS
    new, old = _pair(h, w, 300, 2)
    for inputs, what in ((scene, "degenerate"), (few, "fewer triangles on used plans")):
        want = _want(oracle, inputs, h, w)
        dev = _device(inputs)
        for chain in (new, old):
            chain.bind(dev, flags=flags)
            _rounds(chain, 2)
        for k in range(2):
            _same(new.planes(k), want, f"{what} set {k} against the oracle")
            _same(new.planes(k), old.planes(k), f"{what} set {k} against the general kernel")
    new.close(); old.close()


def test_inputs_rewritten_in_place_and_a_join_mid_burst(oracle):
    """Without CRENDER_STATIC_INPUTS a join voids what was binned ahead: the arrays are rewritten behind it, on the
    caller's stream, and the next frames are the new contents'.  A burst cut by a join goes on with the same scene."""
    h, w, depth = 80, 96, 4
    a, b = _soup(41, 300, w), _soup(42, 300, w)
    want_a, want_b = _want(oracle, a, h, w), _want(oracle, b, h, w)
    dev, dev_b = _device(a), _device(b)
    new = Chain(h, w, 300, depth, True)
    new.bind(dev)
    for _ in range(6):
        new.submit(expect=True)
    new.join()                                   # mid-burst: slots 0 and 1 have come round
    for _ in range(3):
        new.submit(expect=True)
    new.join()
    for k in range(depth):
        _same(new.planes(k), want_a, f"scene a set {k}")
    for t, n in zip(dev, dev_b):
        t.copy_(n)
    new.bind(dev)
    for _ in range(depth + 1):
        new.submit(expect=True)
    new.join()
    for k in range(depth):
        _same(new.planes(k), want_b, f"rewritten in place set {k}")
    new.close()


def test_eligible_and_ineligible_frames_alternate_on_the_same_plans(oracle):
    """Bursts of frames that qualify and of frames that do not — a winner plane, the fused light, a composite frame —
    on the same slots and plans, both chains driven alike: the planes agree after every burst, the plans stay
    consistent, and only the plain frames take the small-scene kernel."""
    capi = _capi()
    h, w, depth = 80, 96, 2
    scenes = [_soup(51 + i, 300, w, size=(2, 24)) for i in range(3)]
    devs = [_device(s) for s in scenes]
    plain = capi.FUSED_CLEAR | capi.OVERLAPPED_FRAMES
    new, old = _pair(h, w, 300, depth, winner=True)
    for chain in (new, old):
        for plan in chain.plans:
            capi.check(chain.lib.crender_plan_set_light(plan.handle, (C.c_float * 3)(*LIGHT)), "light")
    rounds = [(0, plain, False, True), (1, plain, True, False), (2, plain, False, True),
              (0, plain | capi.FUSED_GURO, False, False), (1, plain, False, True),
              (2, capi.OVERLAPPED_FRAMES, False, False), (0, plain, False, True)]
    for r, (s, flags, winner, eligible) in enumerate(rounds):
        for chain in (new, old):
            chain.bind(devs[s], flags=flags, winner=winner)
            for _ in range(2 * depth + 1):
                chain.submit(expect=eligible)
            chain.join()
        for k in range(depth):
            _same(new.planes(k, winner=winner), old.planes(k, winner=winner), f"round {r} set {k}")
            if eligible:
                _same(new.planes(k), _want(oracle, scenes[s], h, w), f"round {r} set {k} against the oracle")
    new.close(); old.close()


def test_a_forced_raster_path_delegates(oracle):
    h, w = 80, 96
    scene = _soup(61, 300, w)
    want = _want(oracle, scene, h, w)
    dev = _device(scene)
    for path in (0, 1):
        new = Chain(h, w, 300, 2, True)
        for plan in new.plans:
            plan.set_raster_path(path)
        new.bind(dev)
        for _ in range(5):
            new.submit(expect=False)
        new.join()
        assert all(plan.last_raster_path() == path for plan in new.plans)
        for k in range(2):
            _same(new.planes(k), want, f"forced path {path} set {k}")
        for plan in new.plans:
            plan.set_raster_path(-1)             # ... and left to the plans again, the frames qualify
        for _ in range(5):
            new.submit()
        new.join()
        if path == 0:
            assert new.lib.crender_frame32_last(new.pipe) == 1
        for k in range(2):
            _same(new.planes(k), want, f"after forced path {path} set {k}")
        new.close()


def test_forty_frames_of_a_moving_model(oracle):
    """The filler's switch: a DeviceModel shifted between frames (the filler joins and re-binds at every rewrite)
    with frame32 on, off and left to the default — the same planes as the oracle's at every pose."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.data_structures import Model, DeviceModel
    from cython3dmodelrenderer_amd.scenes import fit_model
    h, w = 80, 96
    rng = np.random.default_rng(7)
    # a bumpy sheet of 12 x 12 cells, two triangles each: small records (a soup of random faces over random vertices is
    # large triangles, whose frames the plans hand to the pixel owners' kernel)
    g = np.arange(13, dtype=np.float32) / 12 - 0.5
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    vertices = np.concatenate([xy, 0.08 * rng.standard_normal((169, 1)).astype(np.float32)], 1).astype(np.float32)
    i, j = [a.reshape(-1) for a in np.meshgrid(np.arange(12), np.arange(12), indexing="ij")]
    a, b, c, d = i * 13 + j, (i + 1) * 13 + j, (i + 1) * 13 + j + 1, i * 13 + j + 1
    faces = np.concatenate([np.stack([a, c, b], 1), np.stack([a, d, c], 1)]).astype(np.int32)      # (facing the camera)
    model = Model(vertices, faces)
    dm = DeviceModel(model)
    dm.set_uniform_color((40.0, 180.0, 250.0))
    fit_model(dm)
    # (tile=32: left to itself the chain of a frame this small takes 16-pixel tiles)
    fillers = {on: AdvancedPixelBufferFiller(h, w, fov=FOV, tile=32, pipeline=True, pipeline_depth=2, frame32=on)
               for on in (True, False, None)}
    for f in fillers.values():
        f.render_model(dm, clear=True)
    for step in range(40):
        dm.shift([0.01, -0.005, 0.02])
        host = [t.cpu().numpy() for t in (dm._vertices_by_triangles, dm._colors_by_triangles, dm._normals_by_triangles)]
        want = _want(oracle, host, h, w)
        assert (want[0] < 1e6).sum() > 500          # the sheet faces the camera
        for on, f in fillers.items():
            f.render_frame()
            f.render_frame()
            got = [f.get_z_tensor().cpu().numpy(), f.get_color_tensor().cpu().numpy(), f.get_normals_tensor().cpu().numpy()]
            _same(got, want, f"pose {step}, frame32={on}")
            assert f._pipe.frame32_last() == (on is not False and f._frame32)
            for plan in f._pipe.plans:
                _capi().plan_debug_check(plan, f._stream())
