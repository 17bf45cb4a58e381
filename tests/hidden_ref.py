"""Host model of the hidden lines: the statements of include/crender_wire.h (crender_wire_hidden) in vectorised numpy, one
float32 operation per step, over (the winner and z planes, the unprojected triangles and projection matrix, the edge
mask, the line's style).  The GPU tests compare csrc/wireframe.hip's k_wire_hidden with it bit for bit;
tests/test_hidden_cpu.py pins it against a plain loop, by identities, on a hand-built scene and against a float64
evaluation of the depth.

A walked segment is clipped along its major axis before it is expanded, so that a line of 2**30 pixels costs what a row
or column of the frame costs; the steps that leave the frame along the minor axis are dropped afterwards.

``dtype=np.float64`` evaluates lam, ze and the hidden test in double precision from the same float32 projected corners
(``depth`` alone: the classes it leads to may differ at ties)."""
import numpy as np

import tex_ref

MAX_DASH = 64
DOMAIN = np.float32(2.0 ** 30)
NONE, HIDDEN, VISIBLE = 0, 1, 2          # the classes of a pixel: the key plane's values before the second launch


def segments(tri, P, H, W, edges=None, pos_of=None):
    """The walked segments: a dict of arrays [n] — ``i`` (the triangle, caller's order), ``e``, the integer end points
    ``xa, ya, xb, yb`` in walking order, and ``za, zb`` float32, the projected depths at them."""
    tri = np.ascontiguousarray(tri, np.float32)
    T = tri.shape[0]
    empty = {k: np.zeros(0, np.int64) for k in ("i", "e", "xa", "ya", "xb", "yb")}
    empty.update(za=np.zeros(0, np.float32), zb=np.zeros(0, np.float32))
    if T == 0:
        return empty
    bits = np.full(T, 7, np.uint8) if edges is None else np.asarray(edges, np.uint8)
    i = np.repeat(np.arange(T, dtype=np.int64), 3)
    e = np.tile(np.arange(3, dtype=np.int64), T)
    q = i if pos_of is None else np.asarray(pos_of).astype(np.int64)[i]
    keep = (((bits[i] >> e) & 1) == 1) & (q < T)
    i, e, q = i[keep], e[keep], q[keep]
    if not len(i):
        return empty
    with np.errstate(all="ignore"):
        proj = tex_ref.project(tri, P, W, H)
        f = (e + 1) % 3
        a, b = proj[q, e], proj[q, f]
        ok = (tri[q, e, 2] > 0) & (tri[q, f, 2] > 0)
        for c in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]):
            ok &= np.abs(c) < DOMAIN                                   # (false for a NaN and for an infinity)
    i, e, a, b = i[ok], e[ok], a[ok], b[ok]
    xa, ya, xb, yb = (np.rint(c).astype(np.int64) for c in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))      # ties to even
    za, zb = a[:, 2].copy(), b[:, 2].copy()
    swap = (yb < ya) | ((yb == ya) & (xb < xa))
    xa, xb = np.where(swap, xb, xa), np.where(swap, xa, xb)
    ya, yb = np.where(swap, yb, ya), np.where(swap, ya, yb)
    za, zb = np.where(swap, zb, za), np.where(swap, za, zb)
    return dict(i=i, e=e, xa=xa, ya=ya, xb=xb, yb=yb, za=za, zb=zb)


def steps(S, H, W, y0=0, y1=None):
    """The steps of the segments `S` on the frame and in the rows: (n, x, y, t, el, xm) — n indexes into `S`, t is the
    step of el along the major axis, xm says whether that axis is x."""
    y1 = H if y1 is None else y1
    dx, dy = S["xb"] - S["xa"], S["yb"] - S["ya"]
    sx, sy = np.sign(dx), np.sign(dy)
    ax, ay = np.abs(dx), np.abs(dy)
    xm = ax > ay                                                       # ties go to y
    el, es = np.where(xm, ax, ay), np.where(xm, ay, ax)
    a1, b1 = np.where(xm, S["xa"], S["ya"]), np.where(xm, S["ya"], S["xa"])
    sa, sb = np.where(xm, sx, sy), np.where(xm, sy, sx)
    M = np.where(xm, W, H)
    # the window of t in which the major coordinate a1 + sa t is on the frame
    lo = np.where(sa > 0, np.maximum(0, -a1), np.where(sa < 0, np.maximum(0, a1 - (M - 1)), 0))
    hi = np.where(sa > 0, np.minimum(el, M - 1 - a1), np.where(sa < 0, np.minimum(el, a1), el))
    hi = np.where((sa == 0) & ((a1 < 0) | (a1 >= M)), -1, hi)
    cnt = np.maximum(hi - lo + 1, 0)
    n = np.repeat(np.arange(len(cnt)), cnt)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if len(cnt) else np.zeros(0, np.int64)
    t = lo[n] + np.arange(int(cnt.sum())) - first[n]
    k = np.where(el[n] > 0, -((el[n] - 2 * t * es[n]) // (2 * np.maximum(el[n], 1))), 0)
    maj, mnr = a1[n] + sa[n] * t, b1[n] + sb[n] * k
    x, y = np.where(xm[n], maj, mnr), np.where(xm[n], mnr, maj)
    on = (x >= 0) & (x < W) & (y >= max(y0, 0)) & (y < min(y1, H))
    return n[on], x[on], y[on], t[on], el[n][on], xm[n][on]


def depth(S, n, t, el, dtype=np.float32):
    """ze of the steps: lam = t / el (0 for el = 0), ze = za + (zb - za) * lam."""
    d_ = dtype
    with np.errstate(all="ignore"):
        lam = np.where(el > 0, t.astype(d_) / np.maximum(el, 1).astype(d_), d_(0))
        dz = S["zb"].astype(d_) - S["za"].astype(d_)
        return S["za"].astype(d_)[n] + dz[n] * lam


def classes(winner, z, tri, pos_of, P, dash=(4, 4), edges=None, depth_bias=1e-3, use_winner=True, y0=0, y1=None,
            dtype=np.float32, counts=None):
    """uint8 [H, W]: HIDDEN where a drawn hidden step lies and no visible one, VISIBLE where a visible step lies, NONE
    elsewhere.  `counts`, a dict, receives ``segments`` (walked), ``steps`` (on the frame and in the rows), and the
    pixels ``hidden``, ``visible`` and ``gaps`` (a hidden edge runs there, in the stipple's gap, and nothing is marked)."""
    d_ = dtype
    on_px, off_px = int(dash[0]), int(dash[1])
    assert 1 <= on_px <= MAX_DASH and 0 <= off_px <= MAX_DASH
    H, W = winner.shape
    S = segments(tri, P, H, W, edges, pos_of)
    n, x, y, t, el, xm = steps(S, H, W, y0, y1)
    key = np.zeros((H, W), np.uint8)
    gap = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        ze = depth(S, n, t, el, d_)
        hidden = np.asarray(z, np.float32).astype(d_)[y, x] < ze - d_(np.float32(depth_bias))
    if use_winner:
        hidden &= np.asarray(winner)[y, x].astype(np.int64) != S["i"][n]
    c = np.where(xm, x, y)
    drawn = hidden & (c % (on_px + off_px) < on_px)
    np.maximum.at(key, (y[drawn], x[drawn]), HIDDEN)
    np.maximum.at(key, (y[~hidden], x[~hidden]), VISIBLE)
    gap[y[hidden & ~drawn], x[hidden & ~drawn]] = True
    if counts is not None:
        counts.update(segments=int(len(S["i"])), steps=int(len(n)), hidden=int((key == HIDDEN).sum()),
                      visible=int((key == VISIBLE).sum()), gaps=int((gap & (key == NONE)).sum()))
    return key


def hidden_lines(color, winner, z, tri, pos_of, P, line=(0, 0, 0), opacity=0.5, dash=(4, 4), edges=None, depth_bias=1e-3,
                 use_winner=True, y0=0, y1=None, counts=None):
    """(a copy of `color` after crender_wire_hidden over rows y0 .. y1, the classes)."""
    assert 0 <= opacity <= 1
    out = np.array(color, np.float32, copy=True)
    key = classes(winner, z, tri, pos_of, P, dash, edges, depth_bias, use_winner, y0, y1, counts=counts)
    on = key == HIDDEN
    a = np.float32(opacity)
    k = np.float32(1) - a
    L = np.asarray(line, np.float32)
    out[on] = out[on] * k + L[None, :] * a
    return out, key


# ---- a hand-built set of segments, for the CPU and the GPU tests alike ---------------------------------------------

FAR_AWAY = (8, 9)                     # the triangles of `odd_segments` whose lines are too long for the plain loop


def odd_segments():
    """(tri [T, 3, 3] for a 64 x 64 frame under tests/pass_edges.py's `P`, the sorted list of the (i, e) that are
    walked).  Triangles whose half-edges leave the frame on each of the four sides, have length 0, end at a NaN or an
    infinity, at or beyond 2^30, or at z <= 0."""
    import pass_edges
    u = pass_edges.unproject
    WB = HB = 64
    d = np.float32

    def at(pts, z=1.0):
        pts = np.float64(pts)
        return u(pts[:, 0], pts[:, 1], z, WB, HB)
    tris = [
        at([(10, 10), (-30, 20), (20, -25)]),           # 0: leaves through the left and the top
        at([(50, 50), (90, 40), (45, 100)]),            # 1: through the right and the bottom
        at([(-20, 30), (80, 33), (30, 90)]),            # 2: crosses the whole frame
        at([(-5, -5), (-40, -8), (-9, -60)]),           # 3: off the frame altogether: walked, no pixel
        at([(12, 40), (12, 40), (12, 40)]),             # 4: three lines of length 0 on the frame
        at([(30.2, 7.4), (29.8, 6.6), (30.4, 7.3)]),    # 5: rounds to one pixel
        at([(70, 70), (70, 70), (70, 70)]),             # 6: length 0, off the frame
        at([(0, 0), (63, 63), (0, 63)]),                # 7: the corners of the frame; a diagonal (a tie of the axes)
        at([(5, 5), (2.0 ** 29, 11), (9, 2.0 ** 29 + 3)]),        # 8: half a billion steps, inside the domain
        at([(-2.0 ** 29, 20), (2.0 ** 29, 44), (31, -2.0 ** 29)]),  # 9: both ends far away, through the frame
        at([(5, 5), (2.0 ** 30, 11), (9, 30)]),         # 10: a corner AT 2^30: its two half-edges are skipped
        at([(5, 5), (20, -2.0 ** 31), (9, 30)]),        # 11: beyond
        at([(20, 20), (40, 25), (30, 45)]),             # 12: a NaN x (below)
        at([(20, 20), (40, 25), (30, 45)]),             # 13: an infinite y
        at([(20, 20), (40, 25), (30, 45)]),             # 14: z = 0 at corner 1
        at([(20, 20), (40, 25), (30, 45)]),             # 15: z < 0 at corner 2
        at([(20, 20), (40, 25), (30, 45)]),             # 16: a NaN z at corner 0
        at([(20, 20), (40, 25), (30, 45)], z=3.0),      # 17: an ordinary triangle, farther away
    ]
    tri = np.ascontiguousarray(np.stack(tris)).astype(d)
    tri[12, 0, 0] = np.nan
    tri[13, 1, 1] = np.inf
    tri[14, 1, 2] = 0.0
    tri[15, 2, 2] = -1.0
    tri[16, 0, 2] = np.nan
    walked = [(i, e) for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 17) for e in range(3)]
    walked += [(10, 2), (11, 2), (12, 1), (13, 2), (14, 2), (15, 0), (16, 1)]
    return tri, sorted(walked)
