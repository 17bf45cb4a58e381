"""Host model of the drawing as vectors: the statements of include/crender_wire.h (crender_wire_runs_count and
crender_wire_runs_emit) in vectorised numpy, one float32 operation per step, built on tests/hidden_ref.py's ``segments``,
``steps`` and ``depth``: the class of every step with the partner-aware winner rule, the maximal runs per segment in the
order (segment, first step), the end points on the unrounded projected edge, and ``half_edges_once``.  The GPU tests
compare csrc/wireframe.hip's k_wire_runs with it bit for bit; tests/test_line_runs_cpu.py pins it against a plain loop, by
an identity with ``hidden_ref.classes`` and against a float64 evaluation of the end points.

``dtype=np.float64`` evaluates u0, u1 and the two lerps in double precision from the same float32 projected corners
(``ends`` alone: the runs are the float32 model's)."""
import numpy as np

import hidden_ref
import tex_ref

HIDDEN, VISIBLE = hidden_ref.HIDDEN, hidden_ref.VISIBLE
GROUP = 256


def groups(T):
    """crender_wire_runs_groups."""
    if T < 0 or 3 * T > 2 ** 31 - 1:
        return -1
    return -(-3 * T // GROUP)


def unrounded(tri, P, H, W, S, pos_of=None):
    """float32 (xa, ya, xb, yb) [n] of the walked segments `S`: the projected ends, unrounded, in walking order."""
    tri = np.ascontiguousarray(tri, np.float32)
    if not len(S["i"]):
        return tuple(np.zeros(0, np.float32) for _ in range(4))
    i, e = S["i"], S["e"]
    q = i if pos_of is None else np.asarray(pos_of).astype(np.int64)[i]
    with np.errstate(all="ignore"):
        proj = tex_ref.project(tri, P, W, H)
    a, b = proj[q, e], proj[q, (e + 1) % 3]
    ra, rb = np.rint(a[:, :2]).astype(np.int64), np.rint(b[:, :2]).astype(np.int64)
    swap = (rb[:, 1] < ra[:, 1]) | ((rb[:, 1] == ra[:, 1]) & (rb[:, 0] < ra[:, 0]))
    xa, xb = np.where(swap, b[:, 0], a[:, 0]), np.where(swap, a[:, 0], b[:, 0])
    ya, yb = np.where(swap, b[:, 1], a[:, 1]), np.where(swap, a[:, 1], b[:, 1])
    assert (np.rint(xa) == S["xa"]).all() and (np.rint(yb) == S["yb"]).all()       # hidden_ref's own walking order
    return xa, ya, xb, yb


def step_classes(winner, z, S, n, x, y, t, el, partners=None, depth_bias=1e-3, use_winner=True):
    """uint8 [steps]: HIDDEN or VISIBLE for every step ``hidden_ref.steps`` lists (those on the frame and in the rows)."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        ze = hidden_ref.depth(S, n, t, el)
        hidden = np.asarray(z, f32)[y, x] < ze - f32(depth_bias)
    if use_winner:
        w = np.asarray(winner)[y, x].astype(np.int64)
        hidden &= w != S["i"][n]
        if partners is not None:
            v = np.asarray(partners).astype(np.int64)[S["i"][n], S["e"][n]]
            hidden &= ~((v >= 0) & (w == (v >> 1)))
    return np.where(hidden, HIDDEN, VISIBLE).astype(np.uint8)


def line_runs(winner, z, tri, pos_of, P, edges=None, partners=None, depth_bias=1e-3, use_winner=True, y0=0, y1=None,
              dtype=np.float32, counts=None):
    """(runs int32 [N, 4]: (s, t0, t1, class), ends `dtype` [N, 4]: (x0, y0, x1, y1)), ordered by (s, t0).  `counts`, a
    dict, receives ``segments`` (walked), ``steps`` (on the frame and in the rows), ``runs``, ``visible``, ``hidden``,
    ``one_step`` (runs one step long) and ``longest`` (in steps)."""
    d_ = dtype
    H, W = winner.shape
    S = hidden_ref.segments(tri, P, H, W, edges, pos_of)
    n, x, y, t, el, xm = hidden_ref.steps(S, H, W, y0, y1)
    cls = step_classes(winner, z, S, n, x, y, t, el, partners, depth_bias, use_winner)
    if len(n):
        # a run starts where the segment, the class or the sequence of steps breaks (the steps are sorted by (n, t))
        brk = np.ones(len(n), bool)
        brk[1:] = (n[1:] != n[:-1]) | (cls[1:] != cls[:-1]) | (t[1:] != t[:-1] + 1)
        first = np.nonzero(brk)[0]
        last = np.concatenate([first[1:] - 1, [len(n) - 1]])
    else:
        first = last = np.zeros(0, np.int64)
    k = n[first]
    s = 3 * S["i"][k] + S["e"][k]
    t0, t1 = t[first], t[last]
    runs = np.stack([s, t0, t1, cls[first].astype(np.int64)], 1).astype(np.int32).reshape(-1, 4)
    xa, ya, xb, yb = (c[k].astype(d_) for c in unrounded(tri, P, H, W, S, pos_of))
    L = el[first]
    with np.errstate(all="ignore"):
        Lf = np.maximum(L, 1).astype(np.float32).astype(d_)
        u0 = np.where(L > 0, np.maximum(t0.astype(np.float32).astype(d_) - d_(0.5), d_(0)) / Lf, d_(0))
        u1 = np.where(L > 0, np.minimum(t1.astype(np.float32).astype(d_) + d_(0.5), Lf) / Lf, d_(1))
        one = d_(1)
        ends = np.stack([xa * (one - u0) + xb * u0, ya * (one - u0) + yb * u0,
                         xa * (one - u1) + xb * u1, ya * (one - u1) + yb * u1], 1).astype(d_).reshape(-1, 4)
    if counts is not None:
        length = t1 - t0 + 1
        counts.update(segments=int(len(S["i"])), steps=int(len(n)), runs=int(len(runs)), visible=int((runs[:, 3] == VISIBLE).sum()),
                      hidden=int((runs[:, 3] == HIDDEN).sum()), one_step=int((length == 1).sum()),
                      longest=int(length.max()) if len(length) else 0)
    return runs, ends


def group_counts(runs, T):
    """uint32 [groups(T)]: what crender_wire_runs_count writes for these runs."""
    return np.bincount(runs[:, 0] // GROUP, minlength=groups(T)).astype(np.uint32)


def half_edges_once(edges, partners):
    """``wireframe.half_edges_once`` read statement by statement, in a plain loop."""
    partners = np.asarray(partners)
    T = len(partners)
    bits = np.full(T, 7, np.uint8) if edges is None else np.asarray(edges, np.uint8)
    out = bits & 7
    for i in range(T):
        for e in range(3):
            v = int(partners[i, e])
            if not (int(bits[i]) >> e) & 1 or v < 0 or (v >> 1) >= i:
                continue
            p = v >> 1
            if any(int(partners[p, k]) >= 0 and int(partners[p, k]) >> 1 == i and (int(bits[p]) >> k) & 1 for k in range(3)):
                out[i] &= ~(1 << e) & 0xFF
    return out.astype(np.uint8)


# ---- the picket fence: runs that cross a trip of 256 candidates, in one workgroup ------------------------------------

FENCE = 320


def picket_fence():
    """(tri, col, nrm) for a 320 x 320 frame under the fov-45 projection (x' = f x / z with f = 2.4142137, as
    tests/util.py's ``random_soup`` places its triangles): one far triangle at z = 2 and 43 teeth at z = 1 in front of it,
    tooth k at x = 8 + 7 k.  The far triangle's edges alternate between visible and hidden; the teeth's long edges are
    single runs of up to 309 steps."""
    f = 2.4142137

    def u(sx, sy, z):
        x = (np.float64(sx) / (FENCE / 2.0) - 1.0) * z / f
        y = (np.float64(sy) / (FENCE / 2.0) - 1.0) * z / f
        return np.stack([x, y, np.full_like(x, z)], -1)
    tris = [u([4.3, 315.6, 160.2], [20.2, 24.7, 300.4], 2.0)]
    for k in range(43):
        x = 8.0 + 7.0 * k
        tris.append(u([x - 0.5, x + 2.5, x + 1.0], [2.0, 2.0, 310.0], 1.0))
    tri = np.ascontiguousarray(np.stack(tris)).astype(np.float32)
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1.0
    col = np.full_like(tri, 200.0)
    return tri, col, nrm
