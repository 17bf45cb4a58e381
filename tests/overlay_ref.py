"""Host model of the hidden-line overlay: the statements of include/crender_wire.h (crender_wire_overlay) in vectorised
numpy, one float32 operation per step, over (the winner plane, its unprojected triangles and projection matrix, the
edge masks, the line's style).  The GPU tests compare csrc/wireframe.hip's k_wire_overlay with it bit for bit;
tests/test_wire_pass_cpu.py pins it by counts, by identities and against a float64 evaluation.

``dtype=np.float64`` evaluates the distances and the window in double precision from the same float32 projected
corners."""
import numpy as np

import tex_ref

MAX_WIDTH = 64


def distances(winner, tri, P, edges=None, y0=0, y1=None, dtype=np.float32):
    """(ys, xs, t, m, nans): the covered pixels of the rows, their winners (the caller's order), each one's distance to
    the nearest drawn edge line of its winner (+inf where none is drawn or none has a distance), and how many distances
    to drawn edges were NaN (edges of no length, corners that are not finite)."""
    tri = np.ascontiguousarray(tri, np.float32)
    H, W = winner.shape
    ys, xs, t = tex_ref.covered(winner, tri.shape[0], y0, y1)
    proj = tex_ref.project(tri, P, W, H)[t].astype(dtype)
    bits = np.full(len(t), 7, np.uint8) if edges is None else np.asarray(edges, np.uint8)[t]
    fx, fy = xs.astype(dtype), ys.astype(dtype)
    m = np.full(len(t), np.inf, dtype)
    nans = 0
    with np.errstate(all="ignore"):
        for e in range(3):
            a, b = proj[:, e], proj[:, (e + 1) % 3]
            l1, l2 = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
            n = l1 * (fy - b[:, 1]) - l2 * (fx - b[:, 0])
            length = np.sqrt(l1 * l1 + l2 * l2)
            d = np.abs(n) / length
            drawn = ((bits >> e) & 1).astype(bool)
            m = np.where(drawn & (d < m), d, m)                     # (a NaN is never taken)
            nans += int((drawn & np.isnan(d)).sum())
    return ys, xs, t, m, nans


def wire_pass(color, winner, tri, P, width=1.0, line=(255, 255, 255), feather=1.0, opacity=1.0, fill=None, edges=None,
              y0=0, y1=None, counts=None, dtype=np.float32):
    """A copy of `color` after crender_wire_overlay over rows y0 .. y1 (in `dtype`).  `counts`, a dict, receives the
    number of covered pixels, of those with a >= 1 (``full``), with 0 < a < 1 (``partial``), not on a line (``off``)
    — a taken before the opacity — and of NaN distances among the drawn edges' (``nan``)."""
    d_ = dtype
    assert 0 < width <= MAX_WIDTH and 0 < feather <= MAX_WIDTH and 0 <= opacity <= 1
    out = np.array(color, np.float32, copy=True).astype(d_)
    y1 = out.shape[0] if y1 is None else y1
    ys, xs, t, m, nans = distances(winner, tri, P, edges, y0, y1, d_)
    hi = np.float32(width) * np.float32(0.5) + np.float32(feather) * np.float32(0.5)      # on the host, in float32
    with np.errstate(all="ignore"):
        a = (d_(hi) - m) / d_(np.float32(feather))
        on = a > 0
        full = a >= 1
        a = np.where(a > 1, d_(1), a)
        a = a * d_(np.float32(opacity))
        L = np.asarray(line, np.float32).astype(d_)
        base = out[ys, xs] if fill is None else np.broadcast_to(np.asarray(fill, np.float32).astype(d_), (len(t), 3))
        k = d_(1) - a
        blended = base * k[:, None] + L[None, :] * a[:, None]
        if fill is None:
            out[ys[on], xs[on]] = blended[on]
        else:
            out[ys, xs] = np.where(on[:, None], blended, base)
    if counts is not None:
        counts.update(covered=len(t), full=int(full.sum()), partial=int((on & ~full).sum()), off=int((~on).sum()),
                      nan=nans)
    return out

