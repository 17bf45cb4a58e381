"""The drawing as vectors on the GPU (csrc/wireframe.hip's k_wire_runs through AdvancedPixelBufferFiller.line_runs, the two C
entries and Renderer(wireframe={"vector": ...})), bit for bit against the host model of tests/runs_ref.py evaluated on the
oracle's frames and on painted planes (itself pinned in tests/test_line_runs_cpu.py): both tensors, every row, in order.
Every case through a filler also checks that z, normals, the winner plane and the colours were only read."""
import ctypes as C

import numpy as np
import pytest

import contour_ref
import hidden_ref
import pass_edges as E
import runs_ref
from pass_scenes import Scene, TriangleModel, edge_mask, filler, host, lib, trex_fixture  # noqa: F401
from util import assert_bit_equal, random_soup

pytestmark = pytest.mark.gpu

GURO = (0.3, -0.2, 1.0)


def _np(a):
    return a if a is None or isinstance(a, np.ndarray) else host(a)


class _Scene(Scene):
    def want(self, **kw):
        """The model's (runs, ends) on the oracle's frame."""
        return runs_ref.line_runs(self.cam.winner, self.cam.z_buffer, self.tri, None, self.cam.proj_mat, **kw)

    def check(self, f, what, rows=None, counts=None, **kw):
        """Draw, take the runs with `kw` and compare both tensors with the model; the planes were only read."""
        self.draw(f)
        d = f.line_runs(**kw)
        y0, y1 = (0, self.H) if rows is None else rows
        runs, ends = self.want(y0=y0, y1=y1, counts=counts, **{k: _np(v) if k in ("edges", "partners") else v for k, v in kw.items()})
        assert (d.height, d.width) == (self.H, self.W) and len(d) == len(runs), (what, len(d), len(runs))
        assert d.runs.dtype.is_floating_point is False and tuple(d.runs.shape) == (len(runs), 4) == tuple(d.ends.shape)
        assert_bit_equal(host(d.runs), runs, f"{what}: the runs")
        assert_bit_equal(host(d.ends), ends, f"{what}: the ends")
        assert_bit_equal(host(d.visible()), ends[runs[:, 3] == 2], f"{what}: visible()")
        assert_bit_equal(host(d.hidden()), ends[runs[:, 3] == 1], f"{what}: hidden()")
        if rows is None:
            self.check_planes(f, what)
        assert_bit_equal(host(f.get_color_tensor())[y0:y1], self.cam.color_buffer[y0:y1], f"{what}: the colours are only read")
        return runs, ends


trex256 = trex_fixture(_Scene)

# (tests/test_line_runs_cpu.py pins the model to these; recorded from a CPU prototype of the contract)
TREX = {
    "all": dict(segments=41442, steps=133478, runs=43763, visible=17339, hidden=26424, one_step=10366, longest=21),
    "once": dict(segments=20721, steps=66739, runs=21876, visible=8668, hidden=13208),
    "feature": dict(segments=5061, steps=13691, runs=5451, visible=2250, hidden=3201),
}


# ---- 1. T-Rex at 256 x 256: 162 groups ---------------------------------------------------------------------------------

def test_trex_every_mask_rule_and_bias(trex256):
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges, half_edges_once
    s = trex256
    f = filler(256, 256)
    assert runs_ref.groups(len(s.tri)) == 162
    sizes = {}
    for rule in (True, False):
        for bias in (1e-3, 0.0):
            c = {}
            s.check(f, f"T-Rex, all edges, rule {rule}, bias {bias}", counts=c, depth_bias=bias, use_winner=rule)
            sizes[rule, bias] = c
    assert {k: sizes[True, 1e-3][k] for k in TREX["all"]} == TREX["all"]
    assert sizes[True, 0.0]["hidden"] != sizes[False, 0.0]["hidden"]
    partners = edge_partners(s.tri)
    once = half_edges_once(None, partners)
    c = {}
    both = s.check(f, "T-Rex, every edge once, the partner rule", counts=c, edges=once, partners=partners)[0]
    assert {k: c[k] for k in TREX["once"]} == TREX["once"]
    # the partner table changes what is visible, and only with the winner rule
    alone = s.want(edges=once)[0]
    assert len(alone) != len(both) or (alone != both).any()
    s.check(f, "T-Rex, once, the table without the rule", edges=once, partners=partners, use_winner=False)
    c = {}
    import torch
    mask = half_edges_once(feature_edges(s.tri, 30.0), partners)
    s.check(f, "T-Rex, the 30 degree mask once, device operands", counts=c, edges=torch.from_numpy(mask).cuda(),
            partners=torch.from_numpy(partners).cuda())
    assert {k: c[k] for k in TREX["feature"]} == TREX["feature"]
    s.check(f, "T-Rex, a random mask", edges=edge_mask("random", s.tri), depth_bias=0.0)
    s.check(f, "T-Rex, a random mask, partners", edges=edge_mask("random", s.tri, 4), partners=partners)


# ---- 2. the picket fence: one workgroup, 108 trips, runs across a trip ---------------------------------------------------

@pytest.fixture(scope="module")
def fence(oracle):
    s = _Scene(oracle, runs_ref.picket_fence(), runs_ref.FENCE, runs_ref.FENCE)
    assert s.covered > 20000
    return s


def test_the_picket_fence_whole_as_a_strip_and_presorted(fence, oracle):
    s = fence
    n = runs_ref.FENCE
    c = {}
    runs, _ = s.check(filler(n, n), "the fence", counts=c)
    assert (c["segments"], c["steps"], c["runs"], c["visible"], c["hidden"], c["longest"]) == (132, 27614, 304, 218, 86, 309)
    assert runs_ref.groups(len(s.tri)) == 1 and -(-c["steps"] // 256) == 108
    assert [int((runs[:, 0] == e).sum()) for e in range(3)] == [87, 43, 45]
    far = runs[runs[:, 0] == 0]
    assert (far[:-1, 3] != far[1:, 3]).all() and set((far[1:-1, 2] - far[1:-1, 1] + 1).tolist()) <= {3, 4}
    assert ((runs[:, 2] - runs[:, 1] + 1) > 256).sum() >= 40             # runs that no trip of 256 candidates holds
    s.check(filler(n, n, presort=True), "the fence, presorted")
    # a strip of 32 rows: every long run is cut to the rows
    y0, y1 = 30, 62
    strip = _Scene(oracle, (s.tri, s.col, s.nrm), n, n, y0=y0, y1=y1)
    c = {}
    strip.check(filler(n, n, row_strip=(y0, y1)), "the fence, rows 30 .. 61", rows=(y0, y1), counts=c)
    assert c["runs"] == 96 and c["longest"] == 32


def test_a_presorted_filler_with_a_random_mask(oracle):
    seed, T, H, W = 73, 3000, 256, 253
    s = _Scene(oracle, random_soup(np.random.default_rng(seed), T, max(H, W), size_px=(3.0, 60.0)), H, W)
    f = filler(H, W, presort=True)
    mask = edge_mask("random", s.tri, seed)
    runs, _ = s.check(f, "presorted, masked", edges=mask)
    assert f._order is not None and len(runs) > 3000


# ---- 3. through the C entries -------------------------------------------------------------------------------------------

GUARD = 0x5EED5EED


def _entries(lib, winner, z, tri, P, edges=None, partners=None, T=None, pos_of=None, y0=0, y1=None, depth_bias=1e-3, use_winner=True,
             short=0):
    """count, the prefix on the device, emit: (runs, ends, counts).  `short`: emit is given an N that much
    smaller.  A guard row behind both results keeps its bits, and every operand is only read."""
    import torch
    from cython3dmodelrenderer_amd import _capi
    H, W = winner.shape
    T = tri.shape[0] if T is None else T
    y1 = H if y1 is None else y1
    pos_of = None if pos_of is None else np.ascontiguousarray(pos_of).view(np.int32)
    given = (winner, z, tri if len(tri) else None, pos_of, edges, partners)
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in given]
    ptr = [None if a is None else a.data_ptr() for a in dev]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    groups = lib.crender_wire_runs_groups(T)
    assert groups == runs_ref.groups(T)
    counts = torch.full((groups + 1,), GUARD, dtype=torch.int32, device="cuda")
    flags = _capi.WIRE_RUNS_USE_WINNER if use_winner else 0
    head = (ptr[0], ptr[1], ptr[2] if T else None, T, ptr[3], _capi.f32_16(P), ptr[4], ptr[5], depth_bias)
    _capi.check(lib.crender_wire_runs_count(*head, counts.data_ptr(), H, W, y0, y1, flags, st), "crender_wire_runs_count")
    assert int(counts[groups]) == GUARD
    counts = counts[:groups]
    after = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(after[-1]) if groups else 0
    N = total - short
    runs = torch.full((total + 1, 4), GUARD, dtype=torch.int32, device="cuda")
    ends = torch.full((total + 1, 4), -7.25, dtype=torch.float32, device="cuda")
    offsets = (after - counts) if groups else torch.zeros(1, dtype=torch.int64, device="cuda")
    _capi.check(lib.crender_wire_runs_emit(*head, offsets.data_ptr(), N, runs.data_ptr(), ends.data_ptr(), H, W, y0, y1, flags, st),
                "crender_wire_runs_emit")
    torch.cuda.synchronize()
    assert (host(runs[N:]) == GUARD).all() and (host(ends[N:]) == -7.25).all(), "rows at and beyond N keep their bits"
    for a, b, name in zip(dev, given, ("winner", "z", "tri", "pos_of", "edges", "partners")):
        if a is not None:
            assert_bit_equal(host(a), np.ascontiguousarray(b), f"{name} is only read")
    return host(runs[:N]), host(ends[:N]), host(counts).view(np.uint32)


DEPTHS = np.float32([0.5, 0.7, 0.75, 0.8, 0.9, 0.95, 1e6, np.nan, np.inf, -np.inf])


def test_the_odd_segments_on_painted_planes(lib, oracle):
    """tests/hidden_ref.py's hand-built set on a 64 x 64 frame — lines of length 0 (u1 = 1), of half a billion steps,
    through each side of the frame, skipped for a NaN, an infinity, 2^30 or z <= 0 — over a z plane of random depths, NaN,
    infinities and the background's 1e6 and a winner plane of random indices, with a random partner table."""
    tri, walked = hidden_ref.odd_segments()
    T = len(tri)
    rng = np.random.default_rng(7)
    winner = rng.integers(-1, T + 2, (64, 64)).astype(np.int32)
    z = rng.choice(DEPTHS, (64, 64))
    mask = rng.integers(0, 256, T).astype(np.uint8)
    partners = rng.integers(-2, 2 * T, (T, 3)).astype(np.int32)
    seen = 0
    for kw in (dict(), dict(partners=partners), dict(edges=mask, depth_bias=0.0), dict(use_winner=False, partners=partners),
               dict(y0=17, y1=50, partners=partners)):
        runs, ends = runs_ref.line_runs(winner, z, tri, None, E.P, **kw)
        got = _entries(lib, winner, z, tri, E.P, **kw)
        assert_bit_equal(got[0], runs, f"the odd segments, {sorted(kw)}: runs")
        assert_bit_equal(got[1], ends, f"the odd segments, {sorted(kw)}: ends")
        assert_bit_equal(got[2], runs_ref.group_counts(runs, T), f"the odd segments, {sorted(kw)}: counts")
        assert (runs[:, 3] == 1).sum() > 20 and (runs[:, 3] == 2).sum() > 20
        seen += len(runs)
    S = hidden_ref.segments(tri, E.P, 64, 64)
    el = np.maximum(np.abs(S["xb"] - S["xa"]), np.abs(S["yb"] - S["ya"]))
    assert (el == 0).sum() >= 3 and el.max() > 2 ** 29 and seen > 300
    # d_pos_of: the triangles moved, some sent beyond T
    perm = rng.permutation(T).astype(np.uint32)
    moved = np.empty_like(tri)
    moved[perm] = tri
    perm[np.arange(T) % 5 == 3] = T + 7
    runs, ends = runs_ref.line_runs(winner, z, moved, perm, E.P, edges=mask, partners=partners)
    got = _entries(lib, winner, z, moved, E.P, edges=mask, partners=partners, pos_of=perm)
    assert_bit_equal(got[0], runs, "d_pos_of: runs")
    assert_bit_equal(got[1], ends, "d_pos_of: ends")


def test_no_triangles_a_second_group_of_two_segments_and_an_n_too_small(lib, oracle):
    rng = np.random.default_rng(3)
    H = W = 64
    tri = random_soup(rng, 86, 64, size_px=(3.0, 30.0))[0]
    tri[85] = E.unproject(np.float64([10, 50, 30]), np.float64([10, 20, 55]), 1.0, W, H)      # the second group is on the frame
    winner = rng.integers(-1, 88, (H, W)).astype(np.int32)
    z = rng.choice(DEPTHS[:7], (H, W))
    # T = 0: no launch, nothing written
    got = _entries(lib, winner, z, tri, E.P, T=0)
    assert got[0].shape == (0, 4) and got[1].shape == (0, 4) and len(got[2]) == 0
    got = _entries(lib, winner, z, tri[:0], E.P)
    assert got[0].shape == (0, 4)
    # T = 85 is one group, T = 86 a second one with two segments
    assert runs_ref.groups(85) == 1 and runs_ref.groups(86) == 2
    for T in (85, 86):
        runs, ends = runs_ref.line_runs(winner, z, tri[:T], None, E.P)
        got = _entries(lib, winner, z, tri[:T], E.P)
        assert_bit_equal(got[0], runs, f"T = {T}: runs")
        assert_bit_equal(got[1], ends, f"T = {T}: ends")
        assert_bit_equal(got[2], runs_ref.group_counts(runs, T), f"T = {T}: counts")
    assert (runs[:, 0] >= 256).sum() >= 2 and got[2][1] == (runs[:, 0] >= 256).sum()
    # an N one smaller than the total: one run fewer is stored, the row behind them keeps its bits (checked in _entries)
    short = _entries(lib, winner, z, tri, E.P, short=1)
    assert_bit_equal(short[0], runs[:-1], "N - 1: runs")
    assert_bit_equal(short[1], ends[:-1], "N - 1: ends")
    # nothing on the frame: every count is 0
    off = np.ascontiguousarray(E.unproject(rng.uniform(-90, -10, (90, 3)), rng.uniform(-90, -10, (90, 3)), 1.0, W, H))
    got = _entries(lib, winner, z, off, E.P)
    assert got[0].shape == (0, 4) and not got[2].any() and len(got[2]) == 2


def test_a_frame_with_nothing_on_it_returns_empty_tensors_without_an_emit(oracle):
    rng = np.random.default_rng(5)
    tri = np.ascontiguousarray(E.unproject(rng.uniform(-90, -10, (40, 3)), rng.uniform(-90, -10, (40, 3)), 1.0, 64, 64))
    tri[..., :2] *= np.float32(2.0 / 2.4142137)                         # (E.P's scale to the fov-45 filler's: still off the frame)
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1.0
    f = filler(64, 64)
    f.render_arrays(tri, np.full_like(tri, 9.0), nrm, clear=True)
    launched = []
    launch = f._launch_pass
    f._launch_pass = lambda entry, args: (launched.append(entry), launch(entry, args))[1]
    d = f.line_runs()
    assert launched == ["crender_wire_runs_count"]
    assert len(d) == 0 and tuple(d.runs.shape) == (0, 4) == tuple(d.ends.shape) and d.runs.is_cuda and d.ends.is_cuda
    assert tuple(d.visible().shape) == (0, 4) == tuple(d.hidden().shape)


# ---- 4. the Renderer -----------------------------------------------------------------------------------------------------

def test_the_renderer_keeps_the_drawing_of_the_view(trex256):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges, half_edges_once
    s = trex256
    model = TriangleModel(s.tri, s.col, s.nrm)
    f = filler(256, 256)
    r = Renderer(f, GuroIllumination(GURO), on_device=True, wireframe={"contours": True, "feature_angle": 30, "vector": True})
    assert r.line_drawing is None
    r.render(model)
    d = r.line_drawing
    # by hand, on the device
    partners = edge_partners(s.tri)
    static = feature_edges(s.tri, 30.0)
    g = filler(256, 256)
    s.draw(g)
    view = g.contour_edges(partners, static=static, borders=True)
    import torch
    p_dev = torch.from_numpy(partners).cuda()
    hand = g.line_runs(edges=half_edges_once(view, p_dev), partners=p_dev)
    assert len(d) == len(hand) > 1000
    assert_bit_equal(host(d.runs), host(hand.runs), "Renderer(vector=True): runs")
    assert_bit_equal(host(d.ends), host(hand.ends), "Renderer(vector=True): ends")
    # and the model on the host mask of the view
    mask = contour_ref.contour_edges(s.tri, s.cam.proj_mat, 256, 256, partners, static=static, borders=True)[0]
    runs, ends = s.want(edges=half_edges_once(mask, partners), partners=partners)
    assert_bit_equal(host(d.runs), runs, "Renderer(vector=True) against the model: runs")
    assert_bit_equal(host(d.ends), ends, "Renderer(vector=True) against the model: ends")
    # a dict: line_runs' arguments
    r = Renderer(f, GuroIllumination(GURO), on_device=True, wireframe={"feature_angle": 30, "vector": dict(depth_bias=0.0, use_winner=False)})
    r.render(model)
    runs, ends = s.want(edges=half_edges_once(static, partners), partners=partners, depth_bias=0.0, use_winner=False)
    assert_bit_equal(host(r.line_drawing.runs), runs, "vector={...}: runs")
    assert_bit_equal(host(r.line_drawing.ends), ends, "vector={...}: ends")
