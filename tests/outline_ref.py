"""Host model of the outline: the statements of include/crender_wire.h (crender_wire_outline) in vectorised numpy, one
float32 operation per step, over (the winner and z planes, the unprojected triangles and projection matrix, the edge
masks, the line's style).  The GPU tests compare csrc/wireframe.hip's k_wire_outline with it bit for bit;
tests/test_wire_outline_cpu.py pins it by counts, by identities, on a hand-built scene and against a float64 evaluation.

The model loops over the (2 r + 1)^2 offsets with shifted planes of validated winners, the pixel's own winner first; an
offset whose winner is the pixel's own is passed over (a minimum does not change when a value is taken twice).  A
``d_pos_of`` has no place here: a test that uses one hands the model the triangles in the caller's order and a winner
plane without the triangles it sends beyond T.

``dtype=np.float64`` evaluates the distances, the depth test and the window in double precision from the same float32
projected corners."""
import numpy as np

import tex_ref

MAX_WIDTH = 64
MAX_RADIUS = 8


def default_radius(width, feather):
    """``wire_pass``'s radius_px=None: the half width of the ramp's foot, and a pixel for the won pixel nearest to the
    closest point."""
    return int(np.ceil((float(width) + float(feather)) / 2.0)) + 1


def distances(winner, z, tri, P, edges=None, radius_px=2, depth_bias=1e-3, y0=0, y1=None, dtype=np.float32):
    """(m, own, nan): m [H, W], every pixel's distance to the nearest edge segment that counts at it (+inf where none
    does, and outside the rows); own int64 [H, W], the validated winner of the rows' pixels (-1: background, or outside
    the rows); nan bool [H, W], the pixels at which a drawn edge of a candidate had a NaN distance."""
    d_ = dtype
    tri = np.ascontiguousarray(tri, np.float32)
    H, W = winner.shape
    T = tri.shape[0]
    y1 = H if y1 is None else y1
    R = int(radius_px)
    assert 0 <= R <= MAX_RADIUS
    own = np.full((H, W), -1, np.int64)
    rows = np.asarray(winner)[y0:y1]
    ok = (rows >= 0) & (rows < T)
    own[y0:y1][ok] = rows[ok]
    m = np.full((H, W), np.inf, d_)
    nan = np.zeros((H, W), bool)
    if T == 0:
        return m, own, nan
    proj = tex_ref.project(tri, P, W, H).astype(d_)
    bits = np.full(T, 7, np.uint8) if edges is None else np.asarray(edges, np.uint8)
    zp = np.asarray(z, np.float32).astype(d_)
    bias = d_(np.float32(depth_bias))
    pad = np.full((H + 2 * R, W + 2 * R), -1, np.int64)         # a strip does not see across its edge, nor the frame
    pad[R:R + H, R:R + W] = own
    in_rows = np.zeros((H, W), bool)
    in_rows[y0:y1] = True
    offsets = [(0, 0)] + [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if (dy, dx) != (0, 0)]
    with np.errstate(all="ignore"):
        for dy, dx in offsets:
            cand = pad[R + dy:R + dy + H, R + dx:R + dx + W]     # cand[y, x]: the validated winner of (x + dx, y + dy)
            sel = (cand >= 0) & in_rows
            if (dy, dx) != (0, 0):
                sel &= cand != own
            ys, xs = np.nonzero(sel)
            if not len(ys):
                continue
            t = cand[ys, xs]
            mine = own[ys, xs]
            always = (mine < 0) | (t == mine)
            c = proj[t]
            fx, fy = xs.astype(d_), ys.astype(d_)
            zq = zp[ys, xs]
            best = m[ys, xs]
            bad = np.zeros(len(t), bool)
            for e in range(3):
                a, b = c[:, e], c[:, (e + 1) % 3]
                ex, ey = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
                px, py = fx - a[:, 0], fy - a[:, 1]
                s = (px * ex + py * ey) / (ex * ex + ey * ey)
                s = np.where(s < 0, d_(0), s)                   # (selects: a NaN passes both)
                s = np.where(s > 1, d_(1), s)
                qx, qy = a[:, 0] + s * ex, a[:, 1] + s * ey
                cx, cy = fx - qx, fy - qy
                d = np.sqrt(cx * cx + cy * cy)
                ze = a[:, 2] + s * (b[:, 2] - a[:, 2])
                drawn = ((bits[t] >> e) & 1).astype(bool)
                counts = always | ((ze - bias) < zq)
                best = np.where(drawn & counts & (d < best), d, best)       # (a NaN is never taken)
                bad |= drawn & np.isnan(d)
            m[ys, xs] = best
            nan[ys, xs] |= bad
    return m, own, nan


def wire_pass(color, winner, z, tri, P, width=1.0, line=(255, 255, 255), feather=1.0, opacity=1.0, fill=None, edges=None,
              depth_bias=1e-3, radius_px=None, y0=0, y1=None, counts=None, dtype=np.float32, field=None):
    """A copy of `color` after crender_wire_outline over rows y0 .. y1 (in `dtype`).  `radius_px` None is
    ``wire_pass``'s default.  `field`: what ``distances`` returned for the same planes, mask, radius, bias and rows (it
    does not depend on the style).  `counts`, a dict, receives the number of covered pixels of the rows, of background
    pixels on a line (``background_on``), of covered ones (``covered_on``), of pixels with a >= 1 (``full``) and with
    0 < a < 1 (``partial``) — a taken before the opacity — and of pixels that met a NaN distance (``nan``)."""
    d_ = dtype
    assert 0 < width <= MAX_WIDTH and 0 < feather <= MAX_WIDTH and 0 <= opacity <= 1
    out = np.array(color, np.float32, copy=True).astype(d_)
    y1 = out.shape[0] if y1 is None else y1
    radius_px = default_radius(width, feather) if radius_px is None else radius_px
    m, own, nan = distances(winner, z, tri, P, edges, radius_px, depth_bias, y0, y1, d_) if field is None else field
    hi = np.float32(width) * np.float32(0.5) + np.float32(feather) * np.float32(0.5)      # on the host, in float32
    with np.errstate(all="ignore"):
        a = (d_(hi) - m) / d_(np.float32(feather))
        on = a > 0
        full = a >= 1
        a = np.where(a > 1, d_(1), a)
        a = a * d_(np.float32(opacity))
        L = np.asarray(line, np.float32).astype(d_)
        covered = own >= 0
        base = out.copy()
        if fill is not None:
            base[covered] = np.asarray(fill, np.float32).astype(d_)
        k = d_(1) - a
        blended = base * k[..., None] + L[None, None, :] * a[..., None]
        out[on] = blended[on]
        if fill is not None:
            off = covered & ~on
            out[off] = base[off]
    if counts is not None:
        counts.update(covered=int(covered.sum()), background_on=int((on & ~covered).sum()),
                      covered_on=int((on & covered).sum()), full=int(full.sum()), partial=int((on & ~full).sum()),
                      nan=int(nan.sum()))
    return out
