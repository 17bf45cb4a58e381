"""Host model of transparency: the statements of include/crender_peel.h's "Transparency" section in vectorised numpy, one
float32 operation per step.  ``fragments`` enumerates the fragments of a frame (every triangle's pixel box walked, the
rasterizer's coverage test and z, the 64-bit depth key), ``layers`` sorts them per pixel, ``peel_next`` is
crender_peel_next on any given layer, ``shade`` the colours a frame stores for a layer's fragments and ``blend`` one
crender_peel_blend; ``transparency`` chains them as ``AdvancedPixelBufferFiller.transparency_pass`` does.  The GPU tests
compare csrc/peel.hip with it bit for bit; tests/test_peel_cpu.py pins it on the oracle's frames.

``dtype=np.float64`` evaluates the blend's statements in double precision from the same float32 inputs (alpha, the
layers' float32 colours, the background): the yardstick of the blend's rounding."""
import numpy as np

import tex_ref

CLEAR_KEY = np.uint64((0x80000000 | 0x49742400) << 32 | 0xFFFFFFFF)      # make_key(zord(1e6f), KEY_LOW_PRIOR)
MAX_LAYERS = 16


def zord(z):
    """raster_math.h's order-preserving map of a float32 z that is not NaN; -0 maps as +0."""
    z = np.asarray(z, np.float32)
    u = np.where(z == 0, np.float32(0.0), z).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def fragment_key(z, idx):
    return (zord(z).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFE) - np.asarray(idx).astype(np.uint64))


assert CLEAR_KEY == (np.uint64(zord(np.float32(1e6))) << np.uint64(32)) | np.uint64(0xFFFFFFFF)


class Fragments:
    """The fragments of a frame: ``pix`` (y * W + x), ``idx`` (the triangle, in the caller's order), ``z`` float32 and
    ``key`` uint64, one entry per fragment, sorted by (pix, key); ``rank`` is a fragment's place among its pixel's."""

    def __init__(self, pix, idx, z, H, W, T):
        key = fragment_key(z, idx)
        order = np.lexsort((key, pix))
        self.pix, self.idx, self.z, self.key = pix[order], idx[order], z[order], key[order]
        self.H, self.W, self.T = H, W, T
        first = np.r_[True, self.pix[1:] != self.pix[:-1]] if len(pix) else np.zeros(0, bool)
        start = np.maximum.accumulate(np.where(first, np.arange(len(pix)), 0)) if len(pix) else np.zeros(0, np.int64)
        self.rank = np.arange(len(pix)) - start

    def __len__(self):
        return len(self.pix)

    @property
    def depth(self):
        """The most fragments any pixel holds."""
        return int(self.rank.max()) + 1 if len(self) else 0


def fragments(tri, nrm, P, H, W, y0=0, y1=None, pos_of=None):
    """The fragments of the frame of rows y0 .. y1.  `pos_of`: only its ``pos_of[i] < T`` is the model's business, since
    the arrays here are in the caller's order."""
    from oracle import oracle as O
    tri = np.ascontiguousarray(tri, np.float32)
    nrm = np.ascontiguousarray(nrm, np.float32)
    T = tri.shape[0]
    y1 = H if y1 is None else y1
    proj = tex_ref.project(tri, P, W, H) if T else tri
    with np.errstate(all="ignore"):
        back = ((nrm[:, 0, 2] + nrm[:, 1, 2]) + nrm[:, 2, 2]) >= 0          # backface(): true for -0, false for NaN
    if pos_of is not None:
        back = back | (np.asarray(pos_of).astype(np.int64) >= T)
    ts, ys, xs = [], [], []
    for i in np.nonzero(~back)[0]:
        xl, xr, yt, yb = (int(v) for v in O.bbox(proj[i], W, H))
        if xl - xr == 0 or yt - yb == 0:
            continue
        yt, yb = max(yt, y0), min(yb, y1)
        if yt >= yb or xl >= xr:
            continue
        gy, gx = np.mgrid[yt:yb, xl:xr]
        ys.append(gy.ravel())
        xs.append(gx.ravel())
        ts.append(np.full(gy.size, i, np.int64))
    if not ts:
        e = np.zeros(0, np.int64)
        return Fragments(e, e, np.zeros(0, np.float32), H, W, T)
    t, ys, xs = np.concatenate(ts), np.concatenate(ys), np.concatenate(xs)
    with np.errstate(all="ignore"):
        p = proj[t]
        b1, b2, b3 = tex_ref.barycentrics(p, xs, ys)
        z = tex_ref.interp(p[:, 0, 2], p[:, 1, 2], p[:, 2, 2], b1, b2, b3)
        keep = ~((b1 < 0) | (b2 < 0) | (b3 < 0)) & (z == z)
    t, ys, xs, z = t[keep], ys[keep], xs[keep], z[keep]
    keep = fragment_key(z, t) < CLEAR_KEY
    return Fragments((ys * W + xs)[keep].astype(np.int64), t[keep], z[keep].astype(np.float32), H, W, T)


def empty_layer(H, W):
    return np.full((H, W), -1, np.int32), np.full((H, W), 1e6, np.float32)


def layers(frags, n):
    """(winner int32 [n, H, W], z float32 [n, H, W]): layer k holds every pixel's fragment of rank k."""
    winner = np.full((n, frags.H, frags.W), -1, np.int32)
    z = np.full((n, frags.H, frags.W), 1e6, np.float32)
    for k in range(n):
        sel = frags.rank == k
        winner[k].ravel()[frags.pix[sel]] = frags.idx[sel]
        z[k].ravel()[frags.pix[sel]] = frags.z[sel]
    return winner, z


def valid(winner, z, T, pos_of=None):
    """Where a layer names a fragment: its winner is a triangle (under pos_of one that lies in d_tri), its z is not NaN."""
    ok = (winner >= 0) & (winner < T) & ~np.isnan(z)
    if pos_of is not None and T:
        ok &= np.asarray(pos_of).astype(np.int64)[np.clip(winner, 0, T - 1)] < T
    return ok


def peel_next(frags, winner, z, pos_of=None, y0=0, y1=None, out=None):
    """crender_peel_next: the layer behind (winner, z), rows y0 .. y1; the other rows are `out`'s (default: empty)."""
    H, W, T = frags.H, frags.W, frags.T
    y1 = H if y1 is None else y1
    w_out, z_out = empty_layer(H, W) if out is None else (out[0].copy(), out[1].copy())
    w_out[y0:y1], z_out[y0:y1] = -1, np.float32(1e6)
    ok = valid(winner, z, T, pos_of)
    ok[:y0], ok[y1:] = False, False
    K = np.zeros(H * W, np.uint64)
    flat = ok.ravel()
    K[flat] = fragment_key(z.ravel()[flat], winner.ravel()[flat])
    above = flat[frags.pix] & (frags.key > K[frags.pix])
    pix, idx, zz = frags.pix[above], frags.idx[above], frags.z[above]      # still sorted by (pix, key)
    first = np.r_[True, pix[1:] != pix[:-1]] if len(pix) else np.zeros(0, bool)
    w_out.ravel()[pix[first]] = idx[first]
    z_out.ravel()[pix[first]] = zz[first]
    return w_out, z_out


def guro_factor(n, light):
    """raster_math.h's guro_factor on [N, 3] float32 normals; `light` is the flipped, normalised float32 vector."""
    l0, l1, l2 = (np.float32(v) for v in light)
    with np.errstate(all="ignore"):
        s = ((np.float32(0.0) + n[:, 0] * l0) + n[:, 1] * l1) + n[:, 2] * l2
        m = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        f = s / (m + np.float32(1e-6))
        f = np.where(f < 0, np.float32(0.0), f)
        f = np.where(f > 1, np.float32(1.0), f)
    return f.astype(np.float32)


def shade(winner, tri, col, nrm, P, light=None, y0=0, y1=None):
    """float32 [H, W, 3]: shade_fragment's colour of every pixel of the rows whose winner is a triangle (0 elsewhere)."""
    H, W = winner.shape
    out = np.zeros((H, W, 3), np.float32)
    tri = np.ascontiguousarray(tri, np.float32)
    T = tri.shape[0]
    ys, xs, t = tex_ref.covered(winner, T, y0, y1)
    if not len(t):
        return out
    proj = tex_ref.project(tri, P, W, H)
    col, nrm = np.asarray(col, np.float32)[t], np.asarray(nrm, np.float32)[t]
    with np.errstate(all="ignore"):
        b1, b2, b3 = tex_ref.barycentrics(proj[t], xs, ys)
        c = np.stack([tex_ref.interp(col[:, 0, j], col[:, 1, j], col[:, 2, j], b1, b2, b3) for j in range(3)], 1)
        if light is not None:
            n = np.stack([tex_ref.interp(nrm[:, 0, j], nrm[:, 1, j], nrm[:, 2, j], b1, b2, b3) for j in range(3)], 1)
            c = c * guro_factor(n, light)[:, None]
    out[ys, xs] = c
    return out


def clamp_alpha(alpha):
    a = np.asarray(alpha, np.float32)
    with np.errstate(invalid="ignore"):
        a = np.where(a > 0, a, np.float32(0.0))
        return np.where(a > 1, np.float32(1.0), a).astype(np.float32)


def blend(out, trans, winner, T, alpha, colour, first=False, last=False, background=(0, 0, 0), pos_of=None, y0=0, y1=None,
          dtype=np.float32):
    """One crender_peel_blend over rows y0 .. y1, in place on `out` [H, W, 3] and `trans` [H, W] (arrays of `dtype`).
    `colour` float32 [H, W, 3] holds the layer's colours (``shade``, or the front plane), `alpha` float32 [T]."""
    H, W = winner.shape
    y1 = H if y1 is None else y1
    d = dtype
    rows = np.zeros((H, W), bool)
    rows[y0:y1] = True
    is_tri = (winner >= 0) & (winner < T)
    if pos_of is not None and T:
        is_tri &= np.asarray(pos_of).astype(np.int64)[np.clip(winner, 0, T - 1)] < T
    with np.errstate(all="ignore"):
        t = np.ones((H, W), d) if first else trans.copy()
        do = rows & is_tri & (t > 0)
        a = clamp_alpha(np.asarray(alpha, np.float32)[winner[do]]).astype(d) if T else np.zeros(0, d)
        g = t[do] * a
        add = g[:, None] * colour[do].astype(d)
        if first:
            blank = rows & ~do
            out[blank], trans[blank] = 0, 1
            out[do] = add
        else:
            out[do] = out[do] + add
        trans[do] = t[do] * (d(1.0) - a)
        if last:
            left = rows & (trans > 0)
            out[left] = out[left] + trans[left][:, None] * np.asarray(background, np.float32).astype(d)[None, :]
    return out, trans


def transparency(frags, tri, col, nrm, P, alpha, n=4, light=None, background=(0, 0, 0), front=None, pos_of=None, y0=0, y1=None,
                 dtype=np.float32, first_layer=None):
    """``transparency_pass``: [H, W, 3] of `dtype`, rows outside y0 .. y1 zero.  `front`: the colour plane that stands
    for layer 0's colours (``front="plane"``), or None (``front="model"``).  `first_layer`: (winner, z) of layer 0, default
    the fragments' own."""
    H, W, T = frags.H, frags.W, frags.T
    out, trans = np.zeros((H, W, 3), dtype), np.zeros((H, W), dtype)
    alpha = np.broadcast_to(np.asarray(alpha, np.float32), (T,))
    if first_layer is None:
        w0, z0 = layers(frags, 1)
        first_layer = (w0[0], z0[0])
    winner, z = first_layer
    for k in range(n):
        if k:
            winner, z = peel_next(frags, winner, z, pos_of, y0, y1)
        colour = front if k == 0 and front is not None else shade(winner, tri, col, nrm, P, light, y0, y1)
        blend(out, trans, winner, T, alpha, colour, k == 0, k == n - 1, background, pos_of, y0, y1, dtype)
    return out
