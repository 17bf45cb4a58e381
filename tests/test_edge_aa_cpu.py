"""Geometric edge anti-aliasing without a GPU: the header against the binding and the library, the entry point's argument
checks, the host model the GPU tests compare with (tests/edge_aa_ref.py) pinned on hand-built scenes whose coverage is
known exactly, by identities on the oracle's frames, against a plain loop, against a float64 evaluation and against the
exact area of every pixel cell; ``AdvancedPixelBufferFiller.edge_aa``'s protocol on CPU tensors and
``Renderer(antialias=...)``."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import edge_aa_ref
import pass_edges
import tex_ref
from pass_scenes import Frame, capi, fake_filler_base, recording_filler, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from util import LIBRARY_SOURCES, UNIT_KEYS, assert_bit_equal, other_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_AA_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p,
                    C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p]


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_edge_aa_symbol_is_declared_exported_and_bound(capi):
    from cython3dmodelrenderer_amd import _build
    header = open(os.path.join(ROOT, "include", "crender_wire.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert "crender_wire_edge_aa" in declared and declared == set(capi.UNIT_SIGNATURES["wire"])
    assert not declared & other_symbols(capi, "wire")
    res, args = capi.UNIT_SIGNATURES["wire"]["crender_wire_edge_aa"]
    assert res == C.c_int and args == EDGE_AA_ARGTYPES
    assert capi.load().crender_wire_edge_aa.argtypes == EDGE_AA_ARGTYPES
    decl = re.search(r"CRENDER_API int crender_wire_edge_aa\((.*?)\);", header, re.S).group(1)
    params = [" ".join(a.split()) for a in decl.split(",")]
    assert len(params) == len(args) == 15
    assert params == ["const int32_t *d_winner", "const float *d_z", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of",
                      "const float *P16", "const uint8_t *d_edges", "float *d_out", "const float *d_color", "int H", "int W",
                      "int y0", "int y1", "unsigned flags", "void *stream"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert "crender_wire_edge_aa" in set(re.findall(r" T (crender_\w+)", out))
    # the feature lives in the wire unit as it was: no new unit, no new source, no new ABI, the same fingerprint
    assert capi.ABI_VERSION == 6
    assert _build.source_sha16() == "35a9bf480abfca1e"
    assert _build.library_sources() == LIBRARY_SOURCES
    assert list(_build.UNITS) == UNIT_KEYS
    unit = open(os.path.join(_build.SRC_DIR, "wireframe.hip")).read()
    # after the outline, before the contour kernels; the projection and the barycentrics are the rasterizer's, called
    assert unit.index("void k_wire_outline") < unit.index("void k_wire_edge_aa") < unit.index("void k_wire_facing")
    body = unit[unit.index("void k_wire_edge_aa"):unit.index("void k_wire_facing")]
    assert body.count("barycentric(t, ") == 2 and "winner_triangle(" in body and "asm" not in body
    assert not re.search(r"CR_DEV[^\n]*\bwinner_triangle\(", unit) and "project_vertex(" not in unit
    assert "extern __shared__" in body and "wave_any(" in body


def test_edge_aa_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    fake, other = C.c_void_p(0x1000), C.c_void_p(0x2000)      # never dereferenced: every call below fails its checks first

    def edge_aa(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=P, edges=None, out=other, col=fake, H=8, W=8, y0=0, y1=8,
                flags=0):
        return L.crender_wire_edge_aa(win, z, tri, T, pos_of, P, edges, out, col, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(z=None), dict(P=None), dict(out=None), dict(col=None)):
        assert edge_aa(**kw) == E and "is NULL" in text(), kw
    assert edge_aa(tri=None) == E and "NULL with T > 0" in text()
    for bad in (-1, -2 ** 40):
        assert edge_aa(T=bad) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2), dict(H=-2 ** 31)):
        assert edge_aa(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert edge_aa(**kw) == E and "rows outside the frame" in text(), kw
    for flags in (1, 2, 0x80000000):
        assert edge_aa(flags=flags) == E and "unknown flag bits" in text(), flags
    assert edge_aa(out=fake) == E and "d_out is d_color" in text()
    assert edge_aa(out=fake, T=0, tri=None) == E and "d_out is d_color" in text()
    assert text().startswith("crender_wire_edge_aa")
    # T == 0 is no argument error: the call goes on to its launch (which copies the rows: tests/test_edge_aa_gpu.py).  It
    # is made here only where no device could run it, and ends in the runtime's refusal, never in EINVAL.
    if not torch.cuda.is_available():
        assert edge_aa(T=0, tri=None) in (capi.OK, capi.EHIP)
        assert edge_aa(T=0, tri=None, edges=fake, pos_of=fake, H=1, W=1, y1=1) in (capi.OK, capi.EHIP)


# ---- the model by hand: edges whose place in the pixel is known exactly -----------------------------------------

P = pass_edges.P
HB = WB = 64                         # a frame whose half sizes are powers of two: screen coordinates are hit exactly
NEAR_C, FAR_C = np.float32([200.0, 100.0, 50.0]), np.float32([40.0, 80.0, 160.0])


def _half_plane(k, f, vertical, z=1.0):
    """A triangle whose edge 0 is the line x = k + f (or y = k + f), 2048 px long, with its third corner 1024 px to the
    left (above): the barycentric that vanishes on the edge is (k + f - x) / 1024, formed without a rounding.  It covers
    every pixel of the frame with x <= k + f (y <= k + f)."""
    e = k + f
    pts = np.float64([(e, 32 - 1024), (e, 32 + 1024), (e - 1024, 32)])
    if not vertical:
        pts = pts[:, ::-1]
    return pass_edges.unproject(pts[:, 0], pts[:, 1], z, WB, HB)


def _paint(k, vertical, background=-1, z_near=0.75, z_far=1e6, far_color=(0.0, 0.0, 0.0)):
    """(winner, z, colour): triangle 0 on the pixels up to and including column (row) k, `background` on the others."""
    winner = np.full((HB, WB), background, np.int32)
    z = np.full((HB, WB), z_far, np.float32)
    color = np.empty((HB, WB, 3), np.float32)
    color[:] = np.float32(far_color)
    sel = (slice(None), slice(0, k + 1)) if vertical else (slice(0, k + 1), slice(None))
    winner[sel], z[sel], color[sel] = 0, z_near, NEAR_C
    return winner, z, color


def _line(plane, k, vertical, lo=-1, hi=3):
    """The pixels k + lo .. k + hi - 1 across the edge, in a row (column) away from the frame's border."""
    return plane[5, k + lo:k + hi] if vertical else plane[k + lo:k + hi, 5]


@pytest.mark.parametrize("vertical", [True, False])
@pytest.mark.parametrize("f,at_k,at_k1", [(0.25, 0.25, 0.0), (0.75, 0.0, 0.25), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0)])
def test_a_flat_triangle_over_black(oracle, vertical, f, at_k, at_k1):
    """The edge at k + f: pixel k keeps 1/2 - f of the background if f < 1/2, pixel k + 1 takes f - 1/2 of the triangle if
    f > 1/2; exactly, since every operand is a dyadic number."""
    k = 20
    tri = _half_plane(k, f, vertical)[None]
    winner, z, color = _paint(k, vertical)
    out, a, direction = edge_aa_ref.edge_aa(color, winner, z, tri, None, P)
    want_a = np.float32([0.0, at_k, at_k1, 0.0])
    assert_bit_equal(_line(a, k, vertical), want_a, f"a across the edge, f = {f}")
    want = np.stack([NEAR_C, NEAR_C * np.float32(1 - at_k), NEAR_C * np.float32(at_k1), np.zeros(3, np.float32)])
    assert_bit_equal(_line(out, k, vertical), want, f"colours across the edge, f = {f}")
    # pixel k looks ahead (direction 1 or 3), pixel k + 1 looks back (0 or 2)
    ahead, back = (1, 0) if vertical else (3, 2)
    assert list(_line(direction, k, vertical)) == [-1, ahead if at_k else -1, back if at_k1 else -1, -1]
    # the same along the whole edge, and nothing else changes
    changed = (out.view(np.uint32) != color.view(np.uint32)).any(2)
    lines = changed if vertical else changed.T
    assert (lines[:, k] == bool(at_k)).all() and (lines[:, k + 1] == bool(at_k1)).all() and lines.sum() == HB * (bool(at_k) + bool(at_k1))


@pytest.mark.parametrize("vertical", [True, False])
def test_a_near_triangle_in_front_of_a_far_one(oracle, vertical):
    """The far triangle covers the frame; the near one's edge decides from both sides, the far one's edges never."""
    k = 20
    far = pass_edges.unproject(np.float64([-4096, 4096, -4096]), np.float64([-4096, -4096, 4096]), 2.0, WB, HB)
    for f, at_k, at_k1 in ((0.25, 0.25, 0.0), (0.75, 0.0, 0.25), (0.0, 0.5, 0.0), (0.5, 0.0, 0.0)):
        tri = np.ascontiguousarray(np.stack([_half_plane(k, f, vertical), far]))
        winner, z, color = _paint(k, vertical, background=1, z_far=0.875, far_color=FAR_C)
        out, a, _ = edge_aa_ref.edge_aa(color, winner, z, tri, None, P)
        assert_bit_equal(_line(a, k, vertical), np.float32([0.0, at_k, at_k1, 0.0]), f"a, f = {f}")
        want = np.stack([NEAR_C, NEAR_C * np.float32(1 - at_k) + FAR_C * np.float32(at_k),
                         FAR_C * np.float32(1 - at_k1) + NEAR_C * np.float32(at_k1), FAR_C])
        assert_bit_equal(_line(out, k, vertical), want, f"colours, f = {f}")
        # equal z: p is the near one.  From pixel k nothing changes; pixel k + 1 now asks ITS triangle, the far one, in
        # which pixel k lies: no edge between the two, and it is not blended
        flat = np.full_like(z, 0.75)
        _, a_eq, _ = edge_aa_ref.edge_aa(color, winner, flat, tri, None, P)
        assert_bit_equal(_line(a_eq, k, vertical), np.float32([0.0, at_k, 0.0, 0.0]), f"a at equal z, f = {f}")
        # a NaN z at either side: the comparison is false, p is the near one
        odd = z.copy()
        odd[winner == 1] = np.nan
        assert_bit_equal(edge_aa_ref.coverage(winner, odd, tri, None, P)[0], a_eq, "NaN z on the far side")


def test_a_masked_exit_edge_and_a_far_pixel_inside_the_near_triangle(oracle):
    k, f = 20, 0.25
    tri = _half_plane(k, f, True)[None]
    winner, z, color = _paint(k, True)
    full = edge_aa_ref.coverage(winner, z, tri, None, P)[0]
    assert full[5, k] == np.float32(0.25)
    # the exit is through edge 0 (corner 0 -> 1: b3 vanishes there): its bit alone draws it, the two others do not
    assert_bit_equal(edge_aa_ref.coverage(winner, z, tri, None, P, edges=np.uint8([1]))[0], full, "edge 0 alone")
    assert_bit_equal(edge_aa_ref.coverage(winner, z, tri, None, P, edges=np.uint8([0xF9]))[0], full, "bits 3 to 7 are ignored")
    for bits in (0, 2, 4, 6, 0xFE):
        a, direction, boundary = edge_aa_ref.coverage(winner, z, tri, None, P, edges=np.uint8([bits]))
        assert not a.any() and (direction == -1).all() and boundary[:, k].all() and boundary[:, k + 1].all(), bits
    out = edge_aa_ref.edge_aa(color, winner, z, tri, None, P, edges=np.uint8([6]))[0]
    assert_bit_equal(out, color, "the colours, copied")
    # a painted pixel in the middle of the near triangle that names another, farther one: the four pixels around it ask
    # the near triangle, find the far pixel inside it, and are not blended; the pixel itself asks the near triangle too
    far = pass_edges.unproject(np.float64([-4096, 4096, -4096]), np.float64([-4096, -4096, 4096]), 2.0, WB, HB)
    both = np.ascontiguousarray(np.stack([tri[0], far]))
    winner2, z2 = winner.copy(), z.copy()
    winner2[30, 8], z2[30, 8] = 1, 0.875
    a, direction, boundary = edge_aa_ref.coverage(winner2, z2, both, None, P)
    assert boundary[29:32, 7:10].sum() == 5 and not a[29:32, 7:10].any()
    assert_bit_equal(a, full, "as without the painted pixel")
    # winners that name no triangle are background
    winner3 = np.where(winner == 0, 0, 7).astype(np.int32)
    assert_bit_equal(edge_aa_ref.coverage(winner3, z, tri, None, P)[0], full, "a winner beyond T")
    gone = edge_aa_ref.coverage(winner, z, tri, np.uint32([5]), P)
    assert not gone[0].any() and not gone[2].any()                       # d_pos_of sends the only triangle beyond T
    assert not edge_aa_ref.coverage(winner, z, tri[:0], None, P)[2].any()     # T = 0


# ---- identities on the oracle's frames -------------------------------------------------------------------------

class _Frame(Frame):
    def run(self, **kw):
        return edge_aa_ref.edge_aa(self.cam.color_buffer, self.cam.winner, self.cam.z_buffer, self.tri, None, self.cam.proj_mat, **kw)


SOUPS = {51: (4000, 200, 173, (1.0, 40.0)), 71: (3000, 256, 256, (3.0, 50.0))}       # test_wire_pass_cpu.py's scenes

soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)


def _frames(trex, soups):
    return [("trex", trex), ("soup51", soups[51]), ("soup71", soups[71])]


def _differs(winner, T):
    """The pixels with a left, right, upper or lower neighbour on the frame whose validated winner is another."""
    own = edge_aa_ref.validated(winner, T)
    d = np.zeros(own.shape, bool)
    d[:, 1:] |= own[:, 1:] != own[:, :-1]
    d[:, :-1] |= own[:, :-1] != own[:, 1:]
    d[1:] |= own[1:] != own[:-1]
    d[:-1] |= own[:-1] != own[1:]
    return d


def test_the_counts_on_trex(trex):
    """T-Rex at 256^2: the figures the README quotes, with all edges and with the mask of the view's contours over the
    creases of 30 degrees and the borders (tests/contour_ref.py's model of ``contour_edges``)."""
    import contour_ref
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    view = contour_ref.contour_edges(trex.tri, trex.cam.proj_mat, 256, 256, edge_partners(trex.tri),
                                     static=feature_edges(trex.tri, 30.0), borders=True)[0]
    got = {}
    for name, mask in (("all", None), ("contours", view)):
        c = {}
        out, a, _ = trex.run(edges=mask, counts=c)
        print(f"T-Rex 256^2, {name} edges: {c}")
        assert c["boundary"] == int(_differs(trex.cam.winner, len(trex.tri)).sum()) and sum(c["bins"]) == c["blended"]
        assert not np.isnan(out).any()
        got[name] = c
    assert got == COUNTS
    assert 0 < got["contours"]["blended"] < got["all"]["blended"] < got["all"]["boundary"]


# (pinned from this model; a in (0, 1/8], (1/8, 1/4], (1/4, 3/8], (3/8, 1/2])
COUNTS = {"all": dict(boundary=14644, blended=9700, bins=[1948, 2228, 2518, 3006]),
          "contours": dict(boundary=14644, blended=2044, bins=[446, 485, 518, 595])}


def test_identities(trex, soups):
    for name, f in _frames(trex, soups):
        base = f.cam.color_buffer
        T = len(f.tri)
        out, a, direction = f.run()
        assert out.dtype == a.dtype == np.float32
        # a pixel whose four neighbours share its winner is copied bit for bit; a lies in [0, 1/2]
        same = ~_differs(f.cam.winner, T)
        assert same.sum() > 10000 and not a[same].any() and (direction[same] == -1).all()
        assert_bit_equal(out[same], base[same], f"{name}: interior pixels")
        assert (a >= 0).all() and (a <= np.float32(0.5)).all() and ((a != 0) == (direction >= 0)).all()
        assert (a[direction >= 0] > 0).all() and (direction >= 0).sum() > 1000
        assert_bit_equal(out[a == 0], base[a == 0], f"{name}: pixels that are not blended")
        # every output channel lies between the two colours it blends, up to one rounding of each product and the sum
        ys, xs = np.nonzero(direction >= 0)
        step = np.asarray(edge_aa_ref.DIRECTIONS)[direction[ys, xs]]
        mine, theirs = base[ys, xs], base[ys + step[:, 1], xs + step[:, 0]]
        lo, hi = np.minimum(mine, theirs), np.maximum(mine, theirs)
        slack = np.float32(2.0 ** -22) * np.maximum(np.abs(lo), np.abs(hi))
        assert (out[ys, xs] >= lo - slack).all() and (out[ys, xs] <= hi + slack).all(), name
        # all bits set is no mask; no bit set copies the plane; bits 3 to 7 are ignored
        assert_bit_equal(f.run(edges=np.full(T, 7, np.uint8))[0], out, f"{name}: all bits against no mask")
        assert_bit_equal(f.run(edges=np.full(T, 0xFF, np.uint8))[0], out, f"{name}: bits 3 to 7")
        assert_bit_equal(f.run(edges=np.zeros(T, np.uint8))[0], base, f"{name}: an all-zero mask")
        assert_bit_equal(f.run(edges=np.full(T, 0xF8, np.uint8))[0], base, f"{name}: the high bits alone")
        # a mask only takes pixels away, and never changes an a it leaves
        mask = np.random.default_rng(5).integers(0, 8, T).astype(np.uint8)
        _, am, dm = f.run(edges=mask)
        assert ((dm >= 0) <= (direction >= 0)).all() and 0 < (dm >= 0).sum() < (direction >= 0).sum()
        assert (am <= a).all()
        # a background-only frame and T = 0 copy
        nothing = np.full_like(f.cam.winner, -1)
        assert_bit_equal(edge_aa_ref.edge_aa(base, nothing, f.cam.z_buffer, f.tri, None, f.cam.proj_mat)[0], base, "background only")
        assert_bit_equal(edge_aa_ref.edge_aa(base, f.cam.winner, f.cam.z_buffer, f.tri[:0], None, f.cam.proj_mat)[0], base, "T = 0")
        # the caller's order and d_tri's: the triangles moved, the mask where the caller put it
        perm = np.random.default_rng(6).permutation(T).astype(np.uint32)
        moved = np.empty_like(f.tri)
        moved[perm] = f.tri
        got = edge_aa_ref.edge_aa(base, f.cam.winner, f.cam.z_buffer, moved, perm, f.cam.proj_mat, edges=mask)
        assert_bit_equal(got[0], f.run(edges=mask)[0], f"{name}: through d_pos_of")


def test_a_strip_does_not_see_across_its_edge(soups):
    f = soups[71]
    base = f.cam.color_buffer
    y0, y1 = 40, 136
    sentinel = np.full_like(base, -7.0)
    strip, a, _ = f.run(y0=y0, y1=y1, out=sentinel)
    assert (strip[:y0] == -7.0).all() and (strip[y1:] == -7.0).all() and not a[:y0].any() and not a[y1:].any()
    assert not f.run(y0=y0, y1=y1)[0][:y0].any()                          # zeros without a plane to start from
    winner, z, color = f.cam.winner.copy(), f.cam.z_buffer.copy(), base.copy()
    winner[:y0], winner[y1:] = 0, 1
    z[:y0], z[y1:] = -5.0, np.nan
    color[:y0], color[y1:] = 7.5, -2.25
    poisoned = edge_aa_ref.edge_aa(color, winner, z, f.tri, None, f.cam.proj_mat, y0=y0, y1=y1, out=sentinel)[0]
    assert_bit_equal(poisoned, strip, "rows outside the strip are not read")
    whole = f.run()[0]
    assert (whole[y0] != strip[y0]).any() and (whole[y1 - 1] != strip[y1 - 1]).any()
    assert_bit_equal(whole[y0 + 1:y1 - 1], strip[y0 + 1:y1 - 1], "the rows inside see the same neighbours")


# ---- the statements again, a pixel at a time -------------------------------------------------------------------

def _loop_model(color, winner, z, tri, P, edges, rows, cols):
    """The contract read line by line, in plain Python over the pixels rows x cols of the frame, np.float32 scalars
    throughout: (colours, a, direction) of those pixels."""
    f32 = np.float32
    H, W = winner.shape
    T = len(tri)
    proj = tex_ref.project(np.ascontiguousarray(tri, np.float32), P, W, H)
    out = color[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].copy()
    a_plane = np.zeros(out.shape[:2], f32)
    d_plane = np.full(out.shape[:2], -1, np.int8)

    def v(x, y):
        t = int(winner[y, x])
        return t if 0 <= t < T else -1
    with np.errstate(all="ignore"):
        for y in rows:
            for x in cols:
                a, best = f32(0), -1
                wp = v(x, y)
                for k, (dx, dy) in enumerate(edge_aa_ref.DIRECTIONS):
                    qx, qy = x + dx, y + dy
                    if not (0 <= qx < W and 0 <= qy < H):
                        continue
                    wq = v(qx, qy)
                    if wp == wq:
                        continue
                    near_is_q = wq >= 0 and (wp < 0 or bool(z[qy, qx] < z[y, x]))
                    (nx, ny), (fx, fy), w = ((qx, qy), (x, y), wq) if near_is_q else ((x, y), (qx, qy), wp)
                    c = proj[w][None]
                    bn = [b[0] for b in tex_ref.barycentrics(c, np.array([nx]), np.array([ny]))]
                    bf = [b[0] for b in tex_ref.barycentrics(c, np.array([fx]), np.array([fy]))]
                    t, ks = f32(np.inf), 0
                    for j in range(3):
                        if bf[j] < 0:
                            tk = bn[j] / (bn[j] - bf[j])
                            if tk < t:
                                t, ks = tk, j + 1
                    if ks == 0:
                        continue
                    if edges is not None and not (int(edges[w]) >> (ks % 3)) & 1:
                        continue
                    s = t - f32(0.5) if near_is_q else f32(0.5) - t
                    s = f32(0.5) if s > f32(0.5) else s
                    if s > a:
                        a, best = s, k
                if best >= 0:
                    dx, dy = edge_aa_ref.DIRECTIONS[best]
                    kk = f32(1) - a
                    at = (y - rows[0], x - cols[0])
                    out[at] = color[y, x] * kk + color[y + dy, x + dx] * a
                    a_plane[at], d_plane[at] = a, best
    return out, a_plane, d_plane


def test_the_vectorised_model_equals_the_loop(oracle, trex):
    from util import random_soup
    # a window of T-Rex that holds silhouette, creases and background, and a whole small soup; with and without a mask
    rows, cols = range(96, 160), range(64, 128)
    sub = trex.cam.winner[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
    assert (sub >= 0).sum() > 500 and (sub < 0).sum() > 500
    mask = np.random.default_rng(3).integers(0, 8, len(trex.tri)).astype(np.uint8)
    for edges in (None, mask):
        want = _loop_model(trex.cam.color_buffer, trex.cam.winner, trex.cam.z_buffer, trex.tri, trex.cam.proj_mat, edges, rows, cols)
        got = trex.run(edges=edges)
        assert (want[2] >= 0).sum() > 100
        for g, w, what in zip(got, want, ("colours", "a", "direction")):
            assert_bit_equal(g[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1], w, f"T-Rex window, {what}")
    tri, col, nrm = random_soup(np.random.default_rng(17), 150, 48, size_px=(2.0, 20.0))
    cam = oracle.OracleFiller(40, 48, fov=45.0)
    cam.render_arrays(tri, col, nrm)
    assert (cam.winner >= 0).sum() > 300
    mask = np.random.default_rng(4).integers(0, 8, len(tri)).astype(np.uint8)
    for edges in (None, mask):
        want = _loop_model(cam.color_buffer, cam.winner, cam.z_buffer, tri, cam.proj_mat, edges, range(40), range(48))
        got = edge_aa_ref.edge_aa(cam.color_buffer, cam.winner, cam.z_buffer, tri, None, cam.proj_mat, edges=edges)
        assert (got[2] >= 0).sum() > 100
        for g, w, what in zip(got, want, ("colours", "a", "direction")):
            assert_bit_equal(g, w, f"soup 40 x 48, {what}")


# ---- against float64 -------------------------------------------------------------------------------------------

A64_MEASURED = 4.408e-6              # measured with this model: 6.480e-7 on T-Rex, 4.408e-6 on seed 51, 4.361e-6 on seed 71


def test_a_against_float64(trex, soups):
    """The same statements in float64 from the same float32 projected corners, every pixel of the three frames, all
    edges.  a is t - 1/2 or 1/2 - t, and t a quotient of barycentrics that are themselves quotients: three roundings of
    2^-24 each on values below 1, and the cancellation in bn - bf where the two centres lie a pixel apart in a triangle
    tens of pixels across.  No pixel of these frames takes another exit or another direction in float64.  The bound is
    ten times the largest measured difference: the margin is for frames not measured.  A check of the model's
    statements, not a bound on the kernel, which is held to bit equality with the float32 model."""
    worst = 0.0
    for name, f in _frames(trex, soups):
        a32 = f.run()[1]
        a64 = f.run(dtype=np.float64)[1]
        assert a32.dtype == np.float32 and a64.dtype == np.float64 and not np.isnan(a64).any()
        diff = float(np.abs(a32.astype(np.float64) - a64).max())
        print(f"{name}: largest |a - a64| = {diff:.3e}")
        worst = max(worst, diff)
    print(f"largest |a - a64| over the three frames = {worst:.3e} (bound {10 * A64_MEASURED:.3e})")
    assert 0 < worst <= 10 * A64_MEASURED


# ---- analytic ground truth: the exact area of every pixel cell ---------------------------------------------------

def _clip_area(poly, x, y):
    """The area of the convex polygon `poly` [(x, y), ...] inside the cell [x - 1/2, x + 1/2] x [y - 1/2, y + 1/2], in
    float64: Sutherland-Hodgman against the four sides, then the shoelace sum."""
    for axis, bound, keep_below in ((0, x - 0.5, False), (0, x + 0.5, True), (1, y - 0.5, False), (1, y + 0.5, True)):
        out = []
        for i, p in enumerate(poly):
            q = poly[(i + 1) % len(poly)]
            p_in = p[axis] <= bound if keep_below else p[axis] >= bound
            q_in = q[axis] <= bound if keep_below else q[axis] >= bound
            if p_in:
                out.append(p)
            if p_in != q_in:
                u = (bound - p[axis]) / (q[axis] - p[axis])
                out.append((p[0] + u * (q[0] - p[0]), p[1] + u * (q[1] - p[1])))
        poly = out
        if len(poly) < 3:
            return 0.0
    return 0.5 * abs(sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(poly, poly[1:] + poly[:1])))


def _exact_coverage(proj, H, W):
    """float64 [H, W]: the share of every pixel's cell that the (non-overlapping) projected triangles cover."""
    cover = np.zeros((H, W))
    for c in proj.astype(np.float64):
        poly = [(c[k, 0], c[k, 1]) for k in range(3)]
        xs, ys = [p[0] for p in poly], [p[1] for p in poly]
        for y in range(max(0, int(np.floor(min(ys))) - 1), min(H, int(np.ceil(max(ys))) + 2)):
            for x in range(max(0, int(np.floor(min(xs))) - 1), min(W, int(np.ceil(max(xs))) + 2)):
                cover[y, x] += _clip_area(poly, x, y)
    return cover


# screen corners of non-overlapping triangles on a 64 x 64 frame: long shallow edges, steep ones, a thin wedge, a corner
# pointing each way; the last scene's triangles touch along an edge they share
TRUTH_SCENES = {
    "shallow": [[(5.3, 6.2), (58.7, 11.9), (9.1, 29.4)], [(12.6, 36.3), (57.2, 30.8), (48.9, 58.6)]],
    "steep": [[(8.4, 3.7), (15.9, 60.2), (3.2, 55.1)], [(25.3, 5.5), (44.8, 8.1), (33.6, 59.4)], [(50.2, 20.7), (61.3, 44.9), (47.5, 57.8)]],
    "wedge": [[(4.2, 31.6), (59.8, 27.3), (59.1, 35.9)], [(10.5, 5.4), (30.2, 4.8), (18.7, 22.1)], [(36.4, 44.2), (58.3, 59.6), (22.9, 57.5)]],
    "shared": [[(6.5, 8.5), (50.25, 12.75), (20.5, 52.25)], [(50.25, 12.75), (56.5, 55.5), (20.5, 52.25)]],
}


@pytest.mark.parametrize("name", list(TRUTH_SCENES))
def test_the_model_is_nearer_to_the_exact_coverage_than_the_frame(oracle, name):
    """Flat white triangles on black at 64 x 64: the colour a pixel should have is 255 times the covered share of its
    cell.  Mean absolute error over the frame, measured with this model: shallow 0.179 against 3.770 unfiltered (a ratio of
    0.047), steep 0.355 against 5.063 (0.070), wedge 0.434 against 3.870 (0.112), shared 0.049 against 2.565 (0.019).
    Only "smaller" is asserted."""
    H = W = 64
    cam = oracle.OracleFiller(H, W, fov=45.0)
    fx, fy = float(cam.proj_mat[0, 0]), float(cam.proj_mat[1, 1])
    tris = []
    for k, pts in enumerate(TRUTH_SCENES[name]):
        pts = np.float64(pts)
        zv = 1.0 + 0.25 * k
        tris.append(np.stack([(pts[:, 0] / (W / 2.0) - 1.0) * zv / fx, (pts[:, 1] / (H / 2.0) - 1.0) * zv / fy, np.full(3, zv)], 1))
    tri = np.ascontiguousarray(np.stack(tris), np.float32)
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1.0
    cam.render_arrays(tri, np.full_like(tri, 255.0), nrm)
    assert (cam.winner >= 0).sum() > 500
    proj = tex_ref.project(tri, cam.proj_mat, W, H)
    truth = 255.0 * _exact_coverage(proj, H, W)
    assert truth.max() <= 255.0 * (1 + 1e-9) and abs(truth.sum() / 255.0 - sum(
        0.5 * abs((c[1, 0] - c[0, 0]) * (c[2, 1] - c[0, 1]) - (c[2, 0] - c[0, 0]) * (c[1, 1] - c[0, 1])) for c in proj.astype(np.float64))) < 1e-6
    out, a, _ = edge_aa_ref.edge_aa(cam.color_buffer, cam.winner, cam.z_buffer, tri, None, cam.proj_mat)
    before = float(np.abs(cam.color_buffer[..., 0].astype(np.float64) - truth).mean())
    after = float(np.abs(out[..., 0].astype(np.float64) - truth).mean())
    print(f"{name}: mean |colour - exact| {before:.4f} unfiltered, {after:.4f} with the pass, ratio {after / before:.3f}")
    assert (a > 0).sum() > 50
    assert after < before


# ---- the Python layer, on CPU tensors --------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses  # noqa: E402


class FakeFiller(fake_filler_base()):
    """The protocol of the two mixins on CPU tensors; the launch is the host model."""

    def _launch_pass(self, entry, args):
        winner, z, tri, T, pos_of, P, edges, out, color, h, w, y0, y1, flags = args
        self.events.append((entry, T, None if edges is None else edges.numpy().copy(), flags))
        assert color is self.color_buffer and out is not color and (h, w, y0, y1) == (self.h, self.w, self.y0, self.y1)
        got = edge_aa_ref.edge_aa(color.numpy(), winner.numpy(), z.numpy(), np.zeros((0, 3, 3), np.float32) if tri is None else tri.numpy(),
                                  pos_of, P, edges=None if edges is None else edges.numpy(), y0=y0, y1=y1, out=out.numpy())[0]
        out.copy_(torch.from_numpy(got))


def test_edge_aa_returns_a_new_tensor_and_leaves_the_views_as_they_were(soups):
    s = soups[71]
    T = len(s.tri)
    f = FakeFiller(s)
    out = f.edge_aa()
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (s.H, s.W, 3)
    assert f.events == ["push", "settle", ("crender_wire_edge_aa", T, None, 0)]       # edits, then the settle, then the launch
    assert_bit_equal(out.numpy(), s.run()[0], "the model's plane")
    assert not f._host_fresh and not f._host_exposed                     # nobody asked for a view: as stale as before
    assert_bit_equal(f.color_buffer.numpy(), s.cam.color_buffer, "the colour plane is only read")
    # an edit made in a view is carried up first and smoothed; the views stay fresh
    view = f.get_color_buffer()
    assert f._host_fresh and f._host_exposed
    view[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    mask = np.random.default_rng(5).integers(0, 256, T).astype(np.uint8)
    f.events.clear()
    again = f.edge_aa(edges=mask)
    assert again is not out and f._host_fresh and not f._host_exposed
    assert (f.color_buffer[100:140, 100:140] == torch.tensor([10.0, 100.0, 200.0])).all()
    edited = s.cam.color_buffer.copy()
    edited[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    want = edge_aa_ref.edge_aa(edited, s.cam.winner, s.cam.z_buffer, s.tri, None, s.cam.proj_mat, edges=mask)[0]
    assert_bit_equal(again.numpy(), want, "over the edited colours")
    assert (want != s.run(edges=mask)[0]).any() and f.get_color_buffer() is view
    assert np.array_equal(f.events[-1][2], mask)
    # a device tensor as the mask
    f.edge_aa(edges=torch.from_numpy(mask))
    assert np.array_equal(f.events[-1][2], mask)
    # a row strip fills its rows and leaves the others zero
    g = FakeFiller(s, row_strip=(37, 75))
    strip = g.edge_aa().numpy()
    assert not strip[:37].any() and not strip[75:].any()
    assert_bit_equal(strip[37:75], s.run(y0=37, y1=75)[0][37:75], "the strip's rows")


def test_edge_aa_refuses_what_wire_pass_refuses(soups):
    s = soups[71]
    T = len(s.tri)
    f = FakeFiller(s)
    f._pipeline = object()
    with pytest.raises(ValueError, match=r"edge_aa is not available on a swap chain \(pipeline=True\)"):
        f.edge_aa()
    with pytest.raises(ValueError, match="edge_aa needs the winner plane"):
        FakeFiller(s, track_winner=False).edge_aa()
    f = FakeFiller(s)
    f._inputs = None
    with pytest.raises(ValueError, match="edge_aa: no frame has been rendered"):
        f.edge_aa()
    f = FakeFiller(s)
    f._last_flags = 0
    with pytest.raises(ValueError, match="edge_aa: the last frame did not start from cleared buffers"):
        f.edge_aa()
    f = FakeFiller(s)
    for bad, word in ((np.zeros(T - 1, np.uint8), rf"T = {T}.*\({T - 1},\)"), (np.zeros(T, np.int32), rf"T = {T}.*int32"),
                      (np.zeros((T, 3), np.uint8), rf"T = {T}.*\({T}, 3\)"), (torch.zeros(T + 1, dtype=torch.uint8), rf"\({T + 1},\)")):
        with pytest.raises(ValueError, match=word):
            f.edge_aa(edges=bad)
    assert f.events == []                                                 # nothing was pushed, settled or launched
    sig = inspect.signature(DeferredPasses.edge_aa)
    assert list(sig.parameters) == ["self", "edges"] and sig.parameters["edges"].default is None
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    assert AdvancedPixelBufferFiller.edge_aa is DeferredPasses.edge_aa


# ---- the Renderer ----------------------------------------------------------------------------------------------

class _Mesh:
    """What the Renderer reads off a model for the edge masks."""

    def __init__(self, tri):
        self._vertices_by_triangles = tri


# a filler that records what the Renderer asks of it; ``image`` is what its pass returns
IMAGE = torch.arange(8 * 8 * 3, dtype=torch.float32).reshape(8, 8, 3)
_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass contour_edges phong_pass ao_pass shade_guro get_color_tensor get_color_buffer edge_aa",
    returns=dict(contour_edges="view mask", edge_aa=IMAGE), quiet="_push_host_edits synchronize get_normals_buffer", image=IMAGE)


def test_renderer_construction():
    from cython3dmodelrenderer_amd.renderer import Renderer
    names = list(inspect.signature(Renderer.__init__).parameters)
    assert "antialias" in names and inspect.signature(Renderer.__init__).parameters["antialias"].default is None
    assert Renderer(SimpleNamespace(), None).antialias is None

    class Plain:
        pass

    class Smooth:
        def edge_aa(self, edges=None):
            pass

        def resolve(self, s):
            pass
    with pytest.raises(ValueError, match=r"Renderer\(antialias=\.\.\.\) needs a filler with an edge anti-aliasing pass.*Plain has no edge_aa"):
        Renderer(Plain(), None, antialias={})
    with pytest.raises(ValueError, match="antialias.*supersample"):
        Renderer(Smooth(), None, antialias={}, supersample=2)
    with pytest.raises(ValueError, match="Smooth has no contour_edges"):
        Renderer(Smooth(), None, antialias=dict(contours=True))
    with pytest.raises(ValueError, match=r"\['width'\] unknown"):
        Renderer(Smooth(), None, antialias=dict(width=2.0))
    opts = dict(feature_angle=30, borders=False)
    r = Renderer(Smooth(), None, antialias=opts)
    assert r.antialias == opts and r.antialias is not opts
    assert Renderer(Smooth(), None, antialias={}).antialias == {}
    assert Renderer(Smooth(), None, supersample=2).antialias is None


def test_renderer_runs_the_pass_last_and_returns_its_plane():
    import contour_ref
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    tri = contour_ref.place(contour_ref.open_cylinder())
    model = _Mesh(tri)
    guro = GuroIllumination((0.3, -0.2, 1.0))
    # fused, all edges: a cleared frame, the pass last, its tensor handed out
    f = _Recorder()
    r = Renderer(f, guro, on_device="fused", antialias={})
    assert r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "get_color_tensor", "edge_aa"]
    assert f.calls[1][2].get("clear") is True and f.calls[-1] == ("edge_aa", (), {})
    # on the device, after the light and after the wire pass; the contours of the view over the creases, as wireframe's
    f = _Recorder()
    r = Renderer(f, guro, on_device=True, wireframe=dict(width=2.0, feature_angle=30),
                 antialias=dict(contours=True, feature_angle=30))
    assert r.render(model) is f.image and r.render(model) is f.image
    names = [c[0] for c in f.calls]
    assert names == ["set_fused_illumination", "render_model", "shade_guro", "wire_pass", "get_color_tensor", "contour_edges",
                     "edge_aa"] * 2
    assert all(c[2].get("clear") is True for c in f.calls if c[0] == "render_model")
    assert [c[2] for c in f.calls if c[0] == "edge_aa"] == [dict(edges="view mask")] * 2
    (_, a0, k0), (_, a1, k1) = [c for c in f.calls if c[0] == "contour_edges"]
    assert a0[0] is a1[0] is r._smoothed[2] and k0["static"] is k1["static"] is r._smoothed[1]      # once per model
    assert np.array_equal(a0[0], edge_partners(tri)) and np.array_equal(k0["static"], feature_edges(tri, 30))
    assert k0["borders"] is True
    assert r._smoothed[1] is r._wired[1]                                 # the wireframe's mask of the same angle, not a second one
    assert [c[2]["edges"] for c in f.calls if c[0] == "wire_pass"] == [r._wired[1]] * 2
    # another angle is another mask; the partner table is shared either way
    f = _Recorder()
    r = Renderer(f, guro, on_device=True, wireframe=dict(contours=True, feature_angle=30), antialias=dict(contours=True, feature_angle=60))
    r.render(model)
    assert r._smoothed[2] is r._wired[2] and r._smoothed[1] is not r._wired[1]
    assert np.array_equal(r._smoothed[1], feature_edges(tri, 60)) and np.array_equal(r._wired[1], feature_edges(tri, 30))
    # an explicit mask; None and False return a fresh numpy copy of the pass's plane
    explicit = np.full(len(tri), 5, np.uint8)
    for on_device in (None, False):
        f = _Recorder()
        got = Renderer(f, guro, on_device=on_device, antialias=dict(edges=explicit)).render(model)
        assert isinstance(got, np.ndarray) and np.array_equal(got, f.image.numpy())
        assert f.calls[-1] == ("edge_aa", (), dict(edges=explicit)) and [c[0] for c in f.calls].count("edge_aa") == 1
        assert all(c[2].get("clear") is True for c in f.calls if c[0] == "render_model")
    # a PhongIllumination with ambient occlusion: ao, light, lines, and the pass after them all
    f = _Recorder()
    r = Renderer(f, PhongIllumination(position=(0.0, 0.0, 1.0)), on_device=True, ambient_occlusion={}, wireframe={}, antialias={})
    assert r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "ao_pass", "phong_pass", "wire_pass",
                                       "get_color_tensor", "edge_aa"]
    # without the option nothing changes: no pass, the filler's own colours
    f = _Recorder()
    assert Renderer(f, guro, on_device="fused").render(model) == "colour"
    assert "edge_aa" not in [c[0] for c in f.calls] and f.calls[1][2] == dict(clear=True)
