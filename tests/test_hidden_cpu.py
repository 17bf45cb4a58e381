"""The hidden lines without a GPU: the header against the binding and the library, the entry point's argument checks and
their order, the host model the GPU tests compare with (tests/hidden_ref.py) pinned against a plain loop, by identities
on the oracle's frames, on a hand-built frame whose hidden pixels are known exactly and against a float64 evaluation of
the depth; ``AdvancedPixelBufferFiller.hidden_line_pass``'s protocol on CPU tensors and ``Renderer(wireframe={"hidden": ...})``."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import contour_ref
import hidden_ref
import pass_edges
import tex_ref
import wire_ref
from pass_scenes import Frame, capi, fake_filler_base, recording_filler, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from util import UNIT_KEYS, assert_bit_equal, other_symbols, random_soup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_float
HIDDEN_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(F), C.c_void_p, C.POINTER(F), F, C.c_int,
                   C.c_int, F, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p]
NAN, INF = float("nan"), float("inf")
T_TOO_LARGE = ((2 ** 31 - 1) * 256) // 3 + 1


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_hidden_symbol_is_declared_exported_and_bound(capi):
    from cython3dmodelrenderer_amd import _build
    header = open(os.path.join(ROOT, "include", "crender_wire.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert "crender_wire_hidden" in declared and declared == set(capi.UNIT_SIGNATURES["wire"])
    assert not declared & other_symbols(capi, "wire")
    res, args = capi.UNIT_SIGNATURES["wire"]["crender_wire_hidden"]
    assert res == C.c_int and args == HIDDEN_ARGTYPES
    assert capi.load().crender_wire_hidden.argtypes == HIDDEN_ARGTYPES
    decl = re.search(r"CRENDER_API int crender_wire_hidden\((.*?)\);", header, re.S).group(1)
    params = [" ".join(a.split()) for a in decl.split(",")]
    assert len(params) == len(args) == 20
    assert params == ["const int32_t *d_winner", "const float *d_z", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of",
                      "const float *P16", "const uint8_t *d_edges", "const float *line3", "float opacity", "int dash_on",
                      "int dash_off", "float depth_bias", "uint32_t *d_key", "float *d_color", "int H", "int W", "int y0", "int y1",
                      "unsigned flags", "void *stream"]
    # a pointer is bound as an address (or as a host float array), every other parameter by its own C type
    by_type = {"float": F, "int": C.c_int, "int64_t": C.c_int64, "unsigned": C.c_uint}
    for p, a in zip(params, args):
        assert a in (C.c_void_p, C.POINTER(F)) if "*" in p else a is by_type[p.rsplit(" ", 1)[0]], p
    assert re.search(r"#define CRENDER_WIRE_HIDDEN_USE_WINNER 1u\b", header) and capi.WIRE_HIDDEN_USE_WINNER == 1
    assert re.search(r"#define CRENDER_WIRE_MAX_DASH 64\b", header) and capi.WIRE_MAX_DASH == hidden_ref.MAX_DASH == 64
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert "crender_wire_hidden" in set(re.findall(r" T (crender_\w+)", out))
    # the feature lives in the wire unit as it was: no new unit, no new source, no new ABI, the same fingerprint
    assert capi.ABI_VERSION == 6
    assert _build.source_sha16() == "35a9bf480abfca1e"
    assert _build.UNITS["wire"][0] == ["wireframe.hip"]
    assert list(_build.UNITS) == UNIT_KEYS
    unit = open(os.path.join(_build.SRC_DIR, "wireframe.hip")).read()
    # after the contour kernels; the walker and the projection are the file's and the rasterizer's own, called
    assert unit.index("void k_wire_contour_mask") < unit.index("void k_wire_hidden") < unit.index("int wire_window(")
    body = unit[unit.index("void k_wire_hidden"):unit.index("int wire_window(")]
    assert body.count("seg_setup(") == 1 and body.count("seg_pixel(") == 1 and "winner_triangle(" in body and "asm" not in body
    assert "wave_incl_sum(" in body and "extern __shared__" not in body and body.count("atomicMax(") == 2
    assert body.count("atomicExch(") == 1
    assert unit.count("uint32_t seg_setup(") == 1 and unit.count("void seg_pixel(") == 1
    assert not re.search(r"CR_DEV[^\n]*\bwinner_triangle\(", unit) and "project_vertex(" not in unit


def test_hidden_argument_errors_and_their_order_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (F * 16)(*([0.0] * 16))
    black = (F * 3)(0.0, 0.0, 0.0)
    fake = C.c_void_p(0x1000)            # never dereferenced: every call below fails its checks first

    def hidden(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=P, edges=None, line=black, opacity=0.5, on=4, off=4, bias=1e-3,
               key=fake, col=fake, H=8, W=8, y0=0, y1=8, flags=1):
        return L.crender_wire_hidden(win, z, tri, T, pos_of, P, edges, line, opacity, on, off, bias, key, col, H, W, y0, y1,
                                     flags, None)

    def text():
        return L.crender_last_error().decode()

    # one bad argument per check, in the header's order: (keywords, the words of its message)
    checks = [
        (dict(win=None), "is NULL"), (dict(z=None), "is NULL"), (dict(P=None), "is NULL"), (dict(line=None), "is NULL"),
        (dict(key=None), "is NULL"), (dict(col=None), "is NULL"),
        (dict(T=-1), "T is negative"), (dict(tri=None), "d_tri is NULL with T > 0"), (dict(W=-2), "H or W is below 1"),
        (dict(y0=3, y1=3), "rows outside the frame"),
        (dict(H=2 ** 20 + 1), "H or W is above 2^20"),
        (dict(opacity=1.001), "opacity is not in [0, 1]"),
        (dict(line=(F * 3)(0.0, NAN, 0.0)), "line3 is not finite"),
        (dict(on=0), "dash_on is not 1 .. 64 or dash_off is not 0 .. 64"),
        (dict(bias=NAN), "depth_bias is not finite"),
        (dict(flags=2), "unknown flag bits"),
        (dict(T=T_TOO_LARGE), "T is too large"),
    ]
    for kw, words in checks:
        assert hidden(**kw) == E and text() == "crender_wire_hidden: " + (
            "d_winner, d_z, P16, line3, d_key or d_color is NULL" if words == "is NULL" else words), kw
    # more values of each
    for kw in (dict(T=-2 ** 40), dict(H=0), dict(H=-2 ** 31), dict(y0=-1), dict(y1=9), dict(y0=5, y1=2), dict(W=2 ** 20 + 1),
               dict(opacity=-0.001), dict(opacity=NAN), dict(opacity=INF), dict(line=(F * 3)(INF, 0.0, 0.0)),
               dict(line=(F * 3)(0.0, 0.0, -INF)), dict(on=65), dict(on=-1), dict(off=-1), dict(off=65), dict(bias=INF),
               dict(bias=-INF), dict(flags=3), dict(flags=0x80000000), dict(T=2 ** 62)):
        assert hidden(**kw) == E and text().startswith("crender_wire_hidden: "), kw
    # every pair of two checks in one call reports the earlier one
    for a in range(len(checks)):
        for b in range(a + 1, len(checks)):
            (ka, wa), (kb, wb) = checks[a], checks[b]
            if set(ka) & set(kb) or wa == wb:
                continue
            assert hidden(**ka, **kb) == E and wa in text(), (ka, kb, text())
    # what is no error: the ends of every range, with T == 0, which returns before any launch (so without a device too)
    for kw in (dict(), dict(tri=None), dict(opacity=0.0), dict(opacity=1.0), dict(on=1, off=0), dict(on=64, off=64), dict(flags=0),
               dict(bias=-1.0), dict(H=2 ** 20, W=2 ** 20, y1=2 ** 20), dict(y0=7), dict(edges=fake, pos_of=fake, H=1, W=1, y1=1)):
        assert hidden(T=0, **kw) == capi.OK, kw


# ---- the statements again, a step at a time ---------------------------------------------------------------------

def _loop_model(color, winner, z, tri, P, edges=None, pos_of=None, line=(0, 0, 0), opacity=0.5, dash=(4, 4), depth_bias=1e-3,
                use_winner=True, y0=0, y1=None):
    """The contract read line by line in plain Python, np.float32 scalars throughout, the pixels of a line from the
    per-line closed form (tests/wire_ref.py's ``line_pixels``, unclipped): (colours, classes)."""
    f32 = np.float32
    H, W = winner.shape
    y1 = H if y1 is None else y1
    T = len(tri)
    key = np.zeros((H, W), np.uint8)
    out = np.array(color, np.float32, copy=True)
    if T:
        proj = tex_ref.project(np.ascontiguousarray(tri, np.float32), P, W, H)
    period = dash[0] + dash[1]
    with np.errstate(all="ignore"):
        for i in range(T):
            q = i if pos_of is None else int(pos_of[i])
            if q >= T:
                continue
            for e in range(3):
                if edges is not None and not (int(edges[i]) >> e) & 1:
                    continue
                f = (e + 1) % 3
                if not (tri[q, e, 2] > 0 and tri[q, f, 2] > 0):
                    continue
                a, b = proj[q, e], proj[q, f]
                if not all(abs(c) < f32(2.0 ** 30) for c in (a[0], a[1], b[0], b[1])):
                    continue
                pa, pb = (int(np.rint(a[0])), int(np.rint(a[1]))), (int(np.rint(b[0])), int(np.rint(b[1])))
                za, zb = a[2], b[2]
                if (pb[1], pb[0]) < (pa[1], pa[0]):
                    pa, pb, za, zb = pb, pa, zb, za
                assert max(abs(pb[0] - pa[0]), abs(pb[1] - pa[1])) < 4096          # (the loop is for lines near the frame)
                x_major = abs(pb[0] - pa[0]) > abs(pb[1] - pa[1])
                pts = wire_ref.line_pixels(pa, pb)
                el = len(pts) - 1
                dz = zb - za
                for t, (x, y) in enumerate(pts):
                    if not (0 <= x < W and 0 <= y < H and y0 <= y < y1):
                        continue
                    lam = f32(t) / f32(el) if el else f32(0)
                    ze = za + dz * lam
                    hidden = bool(z[y, x] < ze - f32(depth_bias))
                    if hidden and use_winner and int(winner[y, x]) == i:
                        hidden = False
                    if not hidden:
                        key[y, x] = max(key[y, x], 2)
                    elif (x if x_major else y) % period < dash[0]:
                        key[y, x] = max(key[y, x], 1)
    k = f32(1) - f32(opacity)
    for y, x in zip(*np.nonzero(key == 1)):
        out[y, x] = out[y, x] * k + np.asarray(line, f32) * f32(opacity)
    return out, key


def test_the_vectorised_model_equals_the_loop(oracle):
    line = (10.0, 200.0, 90.0)
    for seed, T, H, W, size in ((17, 150, 40, 48, (2.0, 20.0)), (18, 120, 33, 7, (2.0, 30.0)), (19, 6, 1, 1, (1.0, 3.0))):
        tri, col, nrm = random_soup(np.random.default_rng(seed), T, max(H, W), size_px=size)
        cam = oracle.OracleFiller(H, W, fov=45.0)
        cam.render_arrays(tri, col, nrm)
        mask = np.random.default_rng(seed + 1).integers(0, 256, T).astype(np.uint8)
        perm = np.random.default_rng(seed + 2).permutation(T).astype(np.uint32)
        perm[::7] = T + 3                                               # triangles the order sends beyond T
        moved = np.empty_like(tri)
        moved[perm[perm < T]] = tri[perm < T]
        marked = 0
        for kw in (dict(), dict(edges=mask, dash=(3, 2)), dict(use_winner=False, depth_bias=0.0, dash=(1, 0)),
                   dict(edges=mask, dash=(2, 5), y0=H // 3, y1=H // 3 + max(1, H // 2), opacity=0.75),
                   dict(edges=mask, pos_of=perm, dash=(1, 1))):
            arrays = moved if "pos_of" in kw else tri
            want = _loop_model(cam.color_buffer, cam.winner, cam.z_buffer, arrays, cam.proj_mat, line=line, **kw)
            kw = dict(kw)
            got = hidden_ref.hidden_lines(cam.color_buffer, cam.winner, cam.z_buffer, arrays, kw.pop("pos_of", None), cam.proj_mat,
                                          line=line, **kw)
            assert_bit_equal(got[1], want[1], f"seed {seed}, {kw}: classes")
            assert_bit_equal(got[0], want[0], f"seed {seed}, {kw}: colours")
            marked += int((got[1] == 1).sum())
        assert marked >= (0 if H * W == 1 else 20), (seed, marked)


# ---- a frame by hand: a far triangle's edge behind a near quad --------------------------------------------------

P = pass_edges.P                      # x' = 2 x / z, y' = 2 y / z, z' = 1 - 0.25 / z: dyadic on a 64 x 64 frame
HB = WB = 64
ROW, X0, X1 = 30, 4, 60               # the far edge: row 30, columns 4 .. 60, at z = 2 (projected 0.875)
QX0, QX1, QY0, QY1 = 20, 43, 10, 50   # the near quad at z = 1 (projected 0.75)
FAR_Z, NEAR_Z = np.float32(0.875), np.float32(0.75)
PAPER = np.float32([240.0, 230.0, 220.0])


def _hand():
    """(tri, winner, z, colour): triangle 0 is the far one, its edge 0 the far edge; 1 and 2 are the quad."""
    far = pass_edges.unproject(np.float64([X0, X1, 32]), np.float64([ROW, ROW, 60]), 2.0, WB, HB)
    c = [(QX0, QY0), (QX1, QY0), (QX1, QY1), (QX0, QY1)]
    quad = [pass_edges.unproject(np.float64([c[k][0] for k in ks]), np.float64([c[k][1] for k in ks]), 1.0, WB, HB)
            for ks in ((0, 1, 2), (0, 2, 3))]
    tri = np.ascontiguousarray(np.stack([far] + quad))
    proj = tex_ref.project(tri, P, WB, HB)
    assert_bit_equal(proj[0, :2], np.float32([[X0, ROW, 0.875], [X1, ROW, 0.875]]), "the far edge, projected exactly")
    assert_bit_equal(proj[1], np.float32([[QX0, QY0, 0.75], [QX1, QY0, 0.75], [QX1, QY1, 0.75]]), "the quad, projected exactly")
    winner = np.full((HB, WB), -1, np.int32)
    z = np.full((HB, WB), 1e6, np.float32)
    winner[ROW, X0:X1 + 1], z[ROW, X0:X1 + 1] = 0, FAR_Z               # the far triangle shows along its own edge
    winner[QY0:QY1 + 1, QX0:QX1 + 1], z[QY0:QY1 + 1, QX0:QX1 + 1] = 1, NEAR_Z
    color = np.empty((HB, WB, 3), np.float32)
    color[:] = PAPER
    return tri, winner, z, color


FAR_EDGE = np.uint8([1, 0, 0])


def test_the_far_edge_behind_the_quad(oracle):
    tri, winner, z, color = _hand()
    cols = np.arange(WB)
    inside = (cols >= QX0) & (cols <= QX1)
    c = {}
    out, key = hidden_ref.hidden_lines(color, winner, z, tri, None, P, line=(0, 0, 0), opacity=0.5, dash=(1, 0), edges=FAR_EDGE, counts=c)
    # the far edge alone: its pixels inside the quad are hidden, the others visible, nothing else is marked
    assert c["segments"] == 1 and c["steps"] == X1 - X0 + 1
    want = np.zeros((HB, WB), np.uint8)
    want[ROW, X0:X1 + 1] = 2
    want[ROW, inside] = 1
    assert_bit_equal(key, want, "solid: the classes")
    assert c["hidden"] == QX1 - QX0 + 1 == 24 and c["visible"] == 33 and c["gaps"] == 0
    half = color.copy()
    half[ROW, inside] = PAPER * np.float32(0.5)                         # k = 0.5, over black
    assert_bit_equal(out, half, "solid: the colours")
    # the stipple is anchored to the screen: the columns with x % 8 < 4
    c = {}
    key = hidden_ref.classes(winner, z, tri, None, P, dash=(4, 4), edges=FAR_EDGE, counts=c)
    assert list(np.nonzero(key[ROW] == 1)[0]) == [24, 25, 26, 27, 32, 33, 34, 35, 40, 41, 42, 43] and c["gaps"] == 12
    key = hidden_ref.classes(winner, z, tri, None, P, dash=(3, 2), edges=FAR_EDGE)
    assert list(np.nonzero(key[ROW] == 1)[0]) == [x for x in range(QX0, QX1 + 1) if x % 5 < 3]
    assert (key[ROW, ~inside & (cols >= X0) & (cols <= X1)] == 2).all()      # a visible step is marked whatever the stipple says
    # the other half-edge order (corner 1 -> 0, as a neighbour would hold it) walks the same pixels with the same operands
    turned = tri.copy()
    turned[0] = tri[0][[1, 0, 2]]
    assert_bit_equal(hidden_ref.classes(winner, z, turned, None, P, dash=(4, 4), edges=FAR_EDGE),
                     hidden_ref.classes(winner, z, tri, None, P, dash=(4, 4), edges=FAR_EDGE), "the half-edge turned round")
    # with every edge: the quad's own edges are visible on the quad (its depth is not below itself less the bias), and a
    # pixel of the far edge under one of them — the two sides and the diagonal — is no hidden-line pixel
    key = hidden_ref.classes(winner, z, tri, None, P, dash=(1, 0))
    diagonal = {int(x) for x, y in wire_ref.line_pixels((QX0, QY0), (QX1, QY1)) if y == ROW}
    assert len(diagonal) == 1 and QX0 < min(diagonal) < QX1
    assert set(np.nonzero(key[ROW] == 1)[0]) == set(range(QX0 + 1, QX1)) - diagonal
    assert (key[QY0, QX0:QX1 + 1] == 2).all() and (key[QY0:QY1 + 1, QX0] == 2).all() and key[ROW, min(diagonal)] == 2


def test_depths_at_the_tie_and_the_winner_rule(oracle):
    tri, winner, z, color = _hand()
    d = np.float32
    run = dict(dash=(1, 0), edges=FAR_EDGE)
    # ze = 0.875 along the whole edge (both ends at one depth); bias 1/8 puts ze - bias on the quad's depth exactly
    tie = hidden_ref.classes(winner, z, tri, None, P, depth_bias=0.125, **run)
    assert (tie[ROW, X0:X1 + 1] == 2).all()                             # equal is not hidden
    below = z.copy()
    below[ROW, QX0:QX1 + 1:2] = np.nextafter(NEAR_Z, d(-np.inf))        # one ulp nearer, every other column
    got = hidden_ref.classes(winner, z=below, tri=tri, pos_of=None, P=P, depth_bias=0.125, **run)
    assert list(np.nonzero(got[ROW] == 1)[0]) == list(range(QX0, QX1 + 1, 2))
    above = hidden_ref.classes(winner, z, tri, None, P, depth_bias=0.125 - 2.0 ** -23, **run)
    assert list(np.nonzero(above[ROW] == 1)[0]) == list(range(QX0, QX1 + 1))     # ze - bias two ulps of the depth farther: hidden
    # a NaN in the z plane, a NaN bias' worth of depth: never hidden; -inf hides, the background's 1e6 never does
    odd = z.copy()
    odd[ROW, 22], odd[ROW, 23], odd[ROW, 5], odd[ROW, 6] = np.nan, np.inf, -np.inf, 1e6
    got = hidden_ref.classes(winner, odd, tri, None, P, use_winner=False, **run)
    assert list(got[ROW, [22, 23, 5, 6]]) == [2, 2, 1, 2]
    # the winner rule: where the plane names the segment's own triangle the step is visible whatever the depths say
    own = winner.copy()
    own[ROW, 30:36] = 0
    with_rule = hidden_ref.classes(own, z, tri, None, P, use_winner=True, **run)
    without = hidden_ref.classes(own, z, tri, None, P, use_winner=False, **run)
    assert list(np.nonzero(with_rule[ROW] == 1)[0]) == [x for x in range(QX0, QX1 + 1) if not 30 <= x < 36]
    assert list(np.nonzero(without[ROW] == 1)[0]) == list(range(QX0, QX1 + 1))
    # only the segment's OWN triangle: the quad's index there changes nothing
    assert_bit_equal(hidden_ref.classes(winner, z, tri, None, P, use_winner=True, **run), without, "another triangle's index")
    # a strip: rows outside it are neither marked nor blended
    out, key = hidden_ref.hidden_lines(color, winner, z, tri, None, P, dash=(1, 0), y0=ROW + 1, y1=HB)
    assert not key[:ROW + 1].any() and key[ROW + 1:].any()
    assert_bit_equal(out[:ROW + 1], color[:ROW + 1], "rows above the strip")


def test_segments_that_are_skipped_or_clipped(oracle):
    """tests/hidden_ref.py's hand-built set, which tests/test_hidden_gpu.py runs on the device: what is walked, and where."""
    tri, want_walked = hidden_ref.odd_segments()
    S = hidden_ref.segments(tri, P, HB, WB)
    walked = sorted(zip(S["i"].tolist(), S["e"].tolist()))
    assert walked == want_walked
    n, x, y, t, el, xm = hidden_ref.steps(S, HB, WB)
    assert ((x >= 0) & (x < WB) & (y >= 0) & (y < HB)).all() and len(n) > 100
    for side in (x == 0, x == WB - 1, y == 0, y == HB - 1):
        assert side.any()                                               # a line leaves through every side of the frame
    assert el.max() > 2 ** 29                                           # a line of half a billion steps costs its visible part
    lengths = np.maximum(np.abs(S["xb"] - S["xa"]), np.abs(S["yb"] - S["ya"]))
    assert (lengths == 0).sum() >= 3                                    # lines of length 0: one pixel each
    # and the plain loop agrees on the part of the set whose lines are short
    short = np.array([k for k in range(len(tri)) if k not in hidden_ref.FAR_AWAY])
    winner = np.full((HB, WB), -1, np.int32)
    z = np.full((HB, WB), 0.5, np.float32)
    color = np.zeros((HB, WB, 3), np.float32)
    want = _loop_model(color, winner, z, tri[short], P, line=(255, 255, 255))
    got = hidden_ref.hidden_lines(color, winner, z, tri[short], None, P, line=(255, 255, 255))
    assert_bit_equal(got[1], want[1], "the odd segments, classes")
    assert_bit_equal(got[0], want[0], "the odd segments, colours")


# ---- identities on the oracle's frames -------------------------------------------------------------------------

class _Frame(Frame):
    def run(self, **kw):
        return hidden_ref.hidden_lines(self.cam.color_buffer, self.cam.winner, self.cam.z_buffer, self.tri, None, self.cam.proj_mat, **kw)

    def classes(self, **kw):
        return hidden_ref.classes(self.cam.winner, self.cam.z_buffer, self.tri, None, self.cam.proj_mat, **kw)


SOUPS = {51: (4000, 200, 173, (1.0, 40.0)), 71: (3000, 256, 256, (3.0, 50.0))}       # test_wire_pass_cpu.py's scenes

soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)


def _frames(trex, soups):
    return [("trex", trex), ("soup51", soups[51]), ("soup71", soups[71])]


# (pinned from this model, solid lines: the figures the README quotes)
COUNTS = {
    "feature, rule, 1e-3": dict(segments=10122, steps=27382, hidden=2305, visible=2745, gaps=0),
    "all, rule, 0": dict(segments=41442, steps=133478, hidden=3809, visible=10224, gaps=0),
    "all, no rule, 0": dict(segments=41442, steps=133478, hidden=7971, visible=6062, gaps=0),
}


def test_the_counts_on_trex(trex):
    """T-Rex at 256^2, solid lines: the 30 degree mask with the winner rule at bias 1e-3, and all edges at bias 0 with
    and without the rule.  At bias 0 the depths alone call nearly half of the visible edges hidden (an edge lies IN the
    surface it bounds); the rule takes those back."""
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    got = {}
    for name, kw in (("feature, rule, 1e-3", dict(edges=feature_edges(trex.tri, 30.0), depth_bias=1e-3, use_winner=True)),
                     ("all, rule, 0", dict(depth_bias=0.0, use_winner=True)), ("all, no rule, 0", dict(depth_bias=0.0, use_winner=False))):
        c = {}
        trex.classes(dash=(1, 0), counts=c, **kw)
        print(f"T-Rex 256^2, {name}: {c}")
        got[name] = c
    assert got == COUNTS
    assert 0 < got["all, rule, 0"]["hidden"] < got["all, no rule, 0"]["hidden"]
    c = {}
    trex.classes(dash=(4, 4), counts=c, edges=feature_edges(trex.tri, 30.0))
    print(f"T-Rex 256^2, the 30 degree mask dashed (4, 4): {c}")
    assert 0 < c["hidden"] < 2305 and c["visible"] == 2745 and c["gaps"] > 0


def test_identities(trex, soups):
    line = (20.0, 30.0, 250.0)
    for name, f in _frames(trex, soups):
        base = f.cam.color_buffer
        T = len(f.tri)
        out, key = f.run(line=line)
        assert out.dtype == np.float32 and key.dtype == np.uint8 and (key == 1).sum() > 300 and (key == 2).sum() > 300
        assert_bit_equal(out[key != 1], base[key != 1], f"{name}: every pixel but the hidden-line ones keeps its bits")
        assert (out[key == 1].view(np.uint32) != base[key == 1].view(np.uint32)).any()
        assert not np.isnan(out).any()
        # a z plane that is all background: nothing is hidden, the colours are untouched, every walked pixel is visible
        far = np.full_like(f.cam.z_buffer, 1e6)
        o2, k2 = hidden_ref.hidden_lines(base, f.cam.winner, far, f.tri, None, f.cam.proj_mat, line=line)
        assert_bit_equal(o2, base, f"{name}: background only")
        S = hidden_ref.segments(f.tri, f.cam.proj_mat, f.H, f.W)
        n, x, y, *_ = hidden_ref.steps(S, f.H, f.W)
        walked = np.zeros((f.H, f.W), bool)
        walked[y, x] = True
        assert_bit_equal(k2, np.where(walked, 2, 0).astype(np.uint8), f"{name}: every walked pixel is visible")
        assert ((key != 0) <= walked).all()
        # opacity 0 stores the colour back, opacity 1 the line
        assert_bit_equal(f.run(line=line, opacity=0.0)[0], base + np.float32(0) * np.float32(line)[None, None, :], f"{name}: opacity 0")
        assert (f.run(line=line, opacity=1.0)[0][key == 1] == np.float32(line)).all()
        # a solid line marks a superset of any dash, and the visible pixels do not depend on the dash
        solid = f.classes(dash=(3, 0))
        for dash in ((3, 1), (3, 5), (1, 64), (64, 64)):
            some = f.classes(dash=dash)
            assert ((some == 1) <= (solid == 1)).all() and ((some == 2) == (solid == 2)).all(), (name, dash)
            assert (some == 1).sum() < (solid == 1).sum()
        assert_bit_equal(f.classes(dash=(7, 0)), solid, f"{name}: every solid line is the same")
        # all bits set is no mask; no bit set marks nothing; bits 3 to 7 are ignored
        assert_bit_equal(f.classes(edges=np.full(T, 7, np.uint8)), f.classes(), f"{name}: all bits against no mask")
        assert_bit_equal(f.classes(edges=np.full(T, 0xFF, np.uint8)), f.classes(), f"{name}: bits 3 to 7")
        assert not f.classes(edges=np.full(T, 0xF8, np.uint8)).any()
        assert_bit_equal(f.run(edges=np.zeros(T, np.uint8))[0], base, f"{name}: an all-zero mask")
        # T = 0
        assert_bit_equal(hidden_ref.hidden_lines(base, f.cam.winner, f.cam.z_buffer, f.tri[:0], None, f.cam.proj_mat)[0], base, "T = 0")
        # the caller's order and d_tri's: the triangles moved, the mask and the winner rule where the caller put them
        mask = np.random.default_rng(5).integers(0, 8, T).astype(np.uint8)
        perm = np.random.default_rng(6).permutation(T).astype(np.uint32)
        moved = np.empty_like(f.tri)
        moved[perm] = f.tri
        got = hidden_ref.hidden_lines(base, f.cam.winner, f.cam.z_buffer, moved, perm, f.cam.proj_mat, edges=mask, line=line)
        assert_bit_equal(got[0], f.run(edges=mask, line=line)[0], f"{name}: through d_pos_of")
        # a strip sees its rows alone, and in them what the whole frame sees (a step does not look at its neighbours)
        y0, y1 = 37, 75
        strip = f.classes(y0=y0, y1=y1)
        assert not strip[:y0].any() and not strip[y1:].any()
        assert_bit_equal(strip[y0:y1], f.classes()[y0:y1], f"{name}: the strip's rows")


def test_masking_one_half_edge_or_both_gives_the_same_marks(oracle):
    """A closed mesh (tests/contour_ref.py's sphere): every edge has two half-edges, which round to the same end points and
    are walked from the same end with the same depths.  Without the winner rule, which tells the two apart, the marks of
    an edge do not depend on which of its halves the mask names."""
    from cython3dmodelrenderer_amd.wireframe import edge_partners
    tri = contour_ref.place(contour_ref.uv_sphere(), angles=(20.0, 30.0, 0.0))
    T = len(tri)
    partners = edge_partners(tri)
    assert (partners >= 0).all()
    H = W = 128
    cam = oracle.OracleFiller(H, W, fov=45.0)
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1.0
    cam.render_arrays(tri, np.full_like(tri, 200.0), nrm)
    assert (cam.winner >= 0).sum() > 1000
    rng = np.random.default_rng(11)
    both = rng.integers(0, 8, T).astype(np.uint8)
    for t in range(T):                                                  # close the mask under "the other half"
        for e in range(3):
            if (both[t] >> e) & 1:
                p = int(partners[t, e]) >> 1
                pe = [k for k in range(3) if int(partners[p, k]) >> 1 == t and _same_edge(tri, t, e, p, k)]
                both[p] |= 1 << pe[0]
    one = both.copy()
    for t in range(T):                                                  # of every masked edge keep the half of the smaller triangle
        for e in range(3):
            p = int(partners[t, e]) >> 1
            if (one[t] >> e) & 1 and p < t:
                one[t] &= ~(1 << e) & 0xFF
    assert 0 < int(np.unpackbits(one).sum()) < int(np.unpackbits(both).sum())

    def marks(mask, **kw):
        return hidden_ref.classes(cam.winner, cam.z_buffer, tri, None, cam.proj_mat, edges=mask, use_winner=False, **kw)
    for kw in (dict(), dict(dash=(2, 3), depth_bias=0.0)):
        a, b = marks(one, **kw), marks(both, **kw)
        assert (a == 1).sum() > 50 and (a == 2).sum() > 50
        assert_bit_equal(a, b, f"one half against both, {kw}")


def _same_edge(tri, t, e, p, k):
    a = {tri[t, e].tobytes(), tri[t, (e + 1) % 3].tobytes()}
    return a == {tri[p, k].tobytes(), tri[p, (k + 1) % 3].tobytes()}


# ---- against float64 -------------------------------------------------------------------------------------------

ZE64_MEASURED = 3.179e-8             # measured with this model: see the docstring below


def test_the_depth_against_float64(trex, soups):
    """ze of every step of the three frames, all edges, in float32 and in float64 from the same float32 projected depths.
    Three roundings (the quotient, the product, the sum) of 2^-24 relative each on values below 1 — projected z lies in
    (0, 1) in front of the near plane — so a difference of a few 2^-25 is what the formats allow.  Measured with this
    model: 2.980e-08 on T-Rex, 3.179e-08 on seed 51, 3.137e-08 on seed 71.  The bound is ten times the largest: the margin
    is for frames not measured.  A check of the model's statements, not a bound on the kernel, which is held to bit
    equality with the float32 model."""
    worst = 0.0
    for name, f in _frames(trex, soups):
        S = hidden_ref.segments(f.tri, f.cam.proj_mat, f.H, f.W)
        n, x, y, t, el, xm = hidden_ref.steps(S, f.H, f.W)
        z32 = hidden_ref.depth(S, n, t, el)
        z64 = hidden_ref.depth(S, n, t, el, np.float64)
        assert z32.dtype == np.float32 and z64.dtype == np.float64 and len(n) > 50000 and np.isfinite(z64).all()
        diff = float(np.abs(z32.astype(np.float64) - z64).max())
        print(f"{name}: largest |ze - ze64| = {diff:.3e} over {len(n)} steps")
        worst = max(worst, diff)
    print(f"largest |ze - ze64| over the three frames = {worst:.3e} (bound {10 * ZE64_MEASURED:.3e})")
    assert 0 < worst <= 10 * ZE64_MEASURED


# ---- the Python layer, on CPU tensors --------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses  # noqa: E402


class FakeFiller(fake_filler_base()):
    """The protocol of the two mixins on CPU tensors; the launch is the host model."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.keys = []

    def _launch_pass(self, entry, args):
        winner, z, tri, T, pos_of, P, edges, line3, opacity, on, off, bias, key, color, h, w, y0, y1, flags = args
        self.events.append((entry, T, None if edges is None else edges.numpy().copy(), (on, off), flags))
        self.keys.append(key)
        assert color is self.color_buffer and z is self.z_buffer and (h, w, y0, y1) == (self.h, self.w, self.y0, self.y1)
        assert key.dtype == torch.int32 and tuple(key.shape) == (h, w) and not key.any()
        assert all(type(v) is float for v in (opacity, bias)) and type(on) is type(off) is int
        got = hidden_ref.hidden_lines(color.numpy(), winner.numpy(), z.numpy(), np.zeros((0, 3, 3), np.float32) if tri is None else tri.numpy(),
                                      pos_of, P, line=tuple(line3), opacity=opacity, dash=(on, off), depth_bias=bias,
                                      edges=None if edges is None else edges.numpy(), use_winner=bool(flags & 1), y0=y0, y1=y1)[0]
        color.copy_(torch.from_numpy(got))


def test_hidden_line_pass_runs_the_protocol_and_keeps_its_key_plane(soups):
    s = soups[71]
    T = len(s.tri)
    f = FakeFiller(s)
    assert f._hidden_key is None
    view = f.get_color_buffer()
    assert f._host_fresh
    f.events.clear()
    assert f.hidden_line_pass() is None
    assert f.events == ["push", "settle", ("crender_wire_hidden", T, None, (4, 4), 1)]       # edits, then the settle, then the launch
    assert not f._host_fresh                                             # the views are stale: the pass wrote the colours
    assert_bit_equal(f.color_buffer.numpy(), s.run()[0], "the defaults: black, half, (4, 4), bias 1e-3, the winner rule")
    assert f.get_color_buffer() is view and f._host_fresh
    assert_bit_equal(view, s.run()[0], "the view after the next getter")
    # the key plane is allocated once and kept
    mask = np.random.default_rng(5).integers(0, 256, T).astype(np.uint8)
    f.hidden_line_pass(color=(255.0, 0.0, 10.0), opacity=1, dash=(2, 0), edges=mask, depth_bias=0, use_winner=False)
    f.hidden_line_pass(edges=torch.from_numpy(mask), dash=(np.int64(3), np.int32(1)), opacity=np.float32(0.25))
    assert len(f.keys) == 3 and f.keys[0] is f.keys[1] is f.keys[2] is f._hidden_key
    assert np.array_equal(f.events[-1][2], mask) and f.events[-1][3:] == ((3, 1), 1) and f.events[-4][3:] == ((2, 0), 0)
    # a row strip draws in its rows alone
    g = FakeFiller(s, row_strip=(37, 75))
    g.hidden_line_pass(color=(255, 255, 255))
    got = g.color_buffer.numpy()
    assert_bit_equal(got[:37], s.cam.color_buffer[:37], "rows above the strip")
    assert_bit_equal(got, s.run(line=(255, 255, 255), y0=37, y1=75)[0], "the strip")
    assert (got[37:75] != s.cam.color_buffer[37:75]).any()


def test_hidden_line_pass_refuses_before_anything_is_launched(soups):
    s = soups[71]
    T = len(s.tri)
    f = FakeFiller(s)
    f._pipeline = object()
    with pytest.raises(ValueError, match=r"hidden_line_pass is not available on a swap chain \(pipeline=True\)"):
        f.hidden_line_pass()
    with pytest.raises(ValueError, match="hidden_line_pass needs the winner plane"):
        FakeFiller(s, track_winner=False).hidden_line_pass()
    f = FakeFiller(s)
    f._inputs = None
    with pytest.raises(ValueError, match="hidden_line_pass: no frame has been rendered"):
        f.hidden_line_pass()
    f = FakeFiller(s)
    f._last_flags = 0
    with pytest.raises(ValueError, match="hidden_line_pass: the last frame did not start from cleared buffers"):
        f.hidden_line_pass()
    f = FakeFiller(s)
    for kw, word in ((dict(opacity=1.5), "opacity"), (dict(opacity=-0.1), "opacity"), (dict(opacity=NAN), "opacity"),
                     (dict(opacity=True), "opacity"), (dict(opacity="1"), "opacity"),
                     (dict(dash=(0, 4)), "dash"), (dict(dash=(65, 4)), "dash"), (dict(dash=(4, -1)), "dash"), (dict(dash=(4, 65)), "dash"),
                     (dict(dash=4), "dash"), (dict(dash=(4, 4, 4)), "dash"), (dict(dash=(4.0, 4)), "dash"), (dict(dash=(True, 1)), "dash"),
                     (dict(depth_bias=NAN), "depth_bias"), (dict(depth_bias=INF), "depth_bias"), (dict(depth_bias=None), "depth_bias"),
                     (dict(color=(0, 0)), "color"), (dict(color=(0, NAN, 0)), "color"), (dict(color=(0, 0, INF)), "color"),
                     (dict(color=5), "color")):
        with pytest.raises(ValueError, match=word):
            f.hidden_line_pass(**kw)
    for bad, word in ((np.zeros(T - 1, np.uint8), rf"T = {T}.*\({T - 1},\)"), (np.zeros(T, np.int32), rf"T = {T}.*int32"),
                      (torch.zeros(T + 1, dtype=torch.uint8), rf"\({T + 1},\)")):
        with pytest.raises(ValueError, match=word):
            f.hidden_line_pass(edges=bad)
    assert f.events == [] and f._hidden_key is None                      # nothing was pushed, settled, allocated or launched
    sig = inspect.signature(DeferredPasses.hidden_line_pass)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("color", (0, 0, 0)), ("opacity", 0.5), ("dash", (4, 4)), ("edges", None), ("depth_bias", 1e-3), ("use_winner", True)]
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    assert AdvancedPixelBufferFiller.hidden_line_pass is DeferredPasses.hidden_line_pass


# ---- the Renderer ----------------------------------------------------------------------------------------------

class _Mesh:
    """What the Renderer reads off a model for the edge masks."""

    def __init__(self, tri):
        self._vertices_by_triangles = tri


# a filler that records what the Renderer asks of it
_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass hidden_line_pass contour_edges shade_guro resolve get_color_tensor",
    returns=dict(contour_edges="view mask", resolve="resolved"), quiet="_push_host_edits synchronize")


def test_renderer_runs_the_hidden_pass_right_after_the_wire_pass():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    tri = contour_ref.place(contour_ref.open_cylinder())
    model = _Mesh(tri)
    guro = GuroIllumination((0.3, -0.2, 1.0))

    class Plain:
        def wire_pass(self, **kw):
            pass
    with pytest.raises(ValueError, match=r"Renderer\(wireframe=\{'hidden': \.\.\.\}\) needs a filler with a hidden-line pass.*Plain has no hidden_line_pass"):
        Renderer(Plain(), None, wireframe=dict(hidden=True))
    with pytest.raises(ValueError, match="takes True or a dict"):
        Renderer(_Recorder(), None, wireframe=dict(hidden=3))
    assert Renderer(Plain(), None, wireframe=dict(hidden=False)).wireframe == dict(hidden=False)
    # True: the defaults, with the mask of the wire pass
    f = _Recorder()
    r = Renderer(f, guro, on_device=True, wireframe=dict(width=2.0, fill=(255, 255, 255), feature_angle=30, hidden=True))
    assert r.render(model) == "colour"
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "shade_guro", "wire_pass", "hidden_line_pass",
                                       "get_color_tensor"]
    wire, hidden = f.calls[3], f.calls[4]
    assert set(wire[2]) == {"width", "fill", "edges"} and set(hidden[2]) == {"edges"} and hidden[1] == ()
    assert hidden[2]["edges"] is wire[2]["edges"] is r._wired[1] and np.array_equal(r._wired[1], feature_edges(tri, 30))
    # a dict: its arguments; the contours of the view, classified once per frame, go to both
    f = _Recorder()
    opts = dict(color=(90, 90, 90), dash=(2, 2), opacity=1.0)
    r = Renderer(f, guro, on_device="fused", wireframe=dict(contours=True, outline=True, hidden=opts))
    r.render(model)
    r.render(model)
    names = [c[0] for c in f.calls]
    assert names == ["set_fused_illumination", "render_model", "contour_edges", "wire_pass", "hidden_line_pass", "get_color_tensor"] * 2
    for wire, hidden in zip([c for c in f.calls if c[0] == "wire_pass"], [c for c in f.calls if c[0] == "hidden_line_pass"]):
        assert wire[2] == dict(outline=True, edges="view mask") and hidden[2] == dict(opts, edges="view mask")
    assert opts == dict(color=(90, 90, 90), dash=(2, 2), opacity=1.0)    # the caller's dict is not written to
    # an explicit mask of its own wins; without a mask the pass gets None: every edge
    own = np.full(len(tri), 5, np.uint8)
    f = _Recorder()
    Renderer(f, guro, on_device=True, wireframe=dict(feature_angle=30, hidden=dict(edges=own))).render(model)
    assert f.calls[4][0] == "hidden_line_pass" and f.calls[4][2]["edges"] is own
    f = _Recorder()
    Renderer(f, guro, on_device=True, wireframe=dict(hidden={})).render(model)
    assert f.calls[3] == ("wire_pass", (), {}) and f.calls[4] == ("hidden_line_pass", (), dict(edges=None))
    # supersampled: both passes on the supersampled frame, before the resolve
    f = _Recorder()
    assert Renderer(f, guro, on_device=True, supersample=2, wireframe=dict(hidden=True)).render(model) == "resolved"
    assert [c[0] for c in f.calls][-3:] == ["wire_pass", "hidden_line_pass", "resolve"] and f.calls[-1][1] == (2,)
    # without the key nothing changes
    f = _Recorder()
    Renderer(f, guro, on_device=True, wireframe=dict(width=2.0)).render(model)
    assert "hidden_line_pass" not in [c[0] for c in f.calls] and f.calls[3] == ("wire_pass", (), dict(width=2.0))
    assert Renderer(SimpleNamespace(), None).wireframe is None
