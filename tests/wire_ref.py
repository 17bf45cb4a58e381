"""Vectorised host model of the wireframe filler for the tests: the colour plane that
EdgeOnlyPixelBufferFiller.compute_triangle_statistics with LineBresenham leaves after every triangle in
index order, from the closed form of the reference's line (pixel t of a line: the major coordinate
moved by t, the minor one by k(t) = ceil((2 t es - el) / (2 el))), clipped to the frame before it is
expanded, so that lines of 2**30 pixels cost what their visible part costs.  The per-pixel host loop
(LineBresenham) pins it on tests/golden/wire_lines.npz and on small soups (tests/test_wireframe_cpu.py)."""
import numpy as np


def line_pixels(p1, p2):
    """int64 [el + 1, 2] pixel sequence of one line, unclipped."""
    (x1, y1), (x2, y2) = p1, p2
    dx, dy = x2 - x1, y2 - y1
    sx, sy = np.sign(dx), np.sign(dy)
    ax, ay = abs(dx), abs(dy)
    xm = ax > ay
    el, es = (ax, ay) if xm else (ay, ax)
    t = np.arange(el + 1, dtype=np.int64)
    k = -((el - 2 * t * es) // (2 * el)) if el else np.zeros_like(t)
    if xm:
        return np.stack([x1 + sx * t, y1 + sy * k], 1)
    return np.stack([x1 + sx * k, y1 + sy * t], 1)


def _segments(tri, draw_edges):
    """Endpoints (int64 [3 T, 2] each) of segment 3 i + e: edge e, or vertex e as a line of length 0."""
    p = np.trunc(np.asarray(tri, np.float64)[:, :, :2]).astype(np.int64)     # int() of a float32
    a = p.reshape(-1, 2)
    b = (p[:, [1, 2, 0]] if draw_edges else p).reshape(-1, 2)
    return a, b


def _visible(a, b, H, W):
    """Per segment the on-screen pixels: (segment index, x, y) arrays, in segment order."""
    d = b - a
    s = np.sign(d)
    ad = np.abs(d)
    xm = ad[:, 0] > ad[:, 1]
    el = np.where(xm, ad[:, 0], ad[:, 1])
    es = np.where(xm, ad[:, 1], ad[:, 0])
    a1 = np.where(xm, a[:, 0], a[:, 1])
    b1 = np.where(xm, a[:, 1], a[:, 0])
    sa = np.where(xm, s[:, 0], s[:, 1])
    sb = np.where(xm, s[:, 1], s[:, 0])
    Ma = np.where(xm, W, H)
    Mb = np.where(xm, H, W)

    def window(c1, sc, M, lo, hi):
        lo = np.where(sc > 0, np.maximum(lo, -c1), np.where(sc < 0, np.maximum(lo, c1 - (M - 1)), lo))
        hi = np.where(sc > 0, np.minimum(hi, M - 1 - c1), np.where(sc < 0, np.minimum(hi, c1), hi))
        off = (sc == 0) & ((c1 < 0) | (c1 >= M))
        return lo, np.where(off, -1, hi)

    lo, hi = window(a1, sa, Ma, np.zeros_like(el), el)
    klo, khi = window(b1, sb, Mb, np.zeros_like(es), es)
    esd = np.maximum(es, 1)
    lo = np.where(es > 0, np.maximum(lo, (2 * el * klo - el) // (2 * esd) + 1), lo)
    hi = np.where(es > 0, np.minimum(hi, (2 * el * khi + el) // (2 * esd)), hi)
    hi = np.where(klo > khi, -1, hi)
    cnt = np.maximum(hi - lo + 1, 0)
    seg = np.repeat(np.arange(len(a)), cnt)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    t = lo[seg] + np.arange(cnt.sum()) - first[seg]
    k = np.where(el[seg] > 0, -((el[seg] - 2 * t * es[seg]) // (2 * np.maximum(el[seg], 1))), 0)
    maj = a1[seg] + sa[seg] * t
    mnr = b1[seg] + sb[seg] * k
    x = np.where(xm[seg], maj, mnr)
    y = np.where(xm[seg], mnr, maj)
    assert ((x >= 0) & (x < W) & (y >= 0) & (y < H)).all()
    return seg, x, y


def wire_plane(tri, H, W, line_color, draw_edges=True, col=None, base=None):
    """float32 [H, W, 3] colour plane after drawing `tri` (float32 [T, 3, 3]) on `base` (zeros if None);
    `col` (float32 [T, 3, 3]): force_triangle_colors."""
    out = np.zeros((H, W, 3), np.float32) if base is None else np.array(base, np.float32, copy=True)
    if len(tri) == 0:
        return out
    a, b = _segments(tri, draw_edges)
    seg, x, y = _visible(a, b, H, W)
    pix = y * W + x
    last = np.full(H * W, -1, np.int64)
    np.maximum.at(last, pix, seg)           # the last write of the reference's sequence wins
    keep = last[pix] == seg
    flat = out.reshape(-1, 3)
    if col is None:
        flat[pix[keep]] = np.asarray(line_color, np.float32)
    else:
        flat[pix[keep]] = np.asarray(col, np.float32).reshape(-1, 3)[seg[keep]]
    return out


class HostImage:
    """A float32 [H, W, 3] plane with the reference Buffer's set_pixel (buffer.py:66-69)."""

    def __init__(self, H, W, base=None):
        self.H, self.W = H, W
        self.a = np.zeros((H, W, 3), np.float32) if base is None else np.array(base, np.float32, copy=True)

    def set_pixel(self, x, y, value):
        if 0 <= x < self.W and 0 <= y < self.H:
            self.a[y, x] = value
