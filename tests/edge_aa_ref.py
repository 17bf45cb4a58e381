"""Host model of the geometric edge anti-aliasing: the statements of include/crender_wire.h (crender_wire_edge_aa) in
vectorised numpy, one float32 operation per step, over (the colour, winner and z planes, the unprojected triangles, a
``d_pos_of``, the projection matrix, the edge mask, the rows).  The GPU tests compare csrc/wireframe.hip's k_wire_edge_aa
with it bit for bit; tests/test_edge_aa_cpu.py pins it by hand-built scenes, by identities, against a plain loop, against
a float64 evaluation and against exact pixel coverage.

The projection and the barycentrics are the existing models' (``tex_ref.project``, ``tex_ref.barycentrics``), imported and
not restated.  ``dtype=np.float64`` evaluates the barycentrics, the exits and the blend in double precision from the same
float32 projected corners (the decision by z is a comparison of the float32 plane either way)."""
import numpy as np

import tex_ref

DIRECTIONS = ((-1, 0), (1, 0), (0, -1), (0, 1))          # (dx, dy), in the contract's order


def validated(winner, T, pos_of=None, y0=0, y1=None):
    """int64 [H, W]: the validated winner of the rows' pixels, -1 elsewhere (the outline's rule)."""
    winner = np.asarray(winner)
    H, W = winner.shape
    y1 = H if y1 is None else y1
    own = np.full((H, W), -1, np.int64)
    rows = winner[y0:y1].astype(np.int64)
    ok = (rows >= 0) & (rows < T)
    if pos_of is not None and T:
        ok &= np.asarray(pos_of).astype(np.int64)[np.clip(rows, 0, T - 1)] < T
    own[y0:y1][ok] = rows[ok]
    return own


def coverage(winner, z, tri, pos_of, P, edges=None, y0=0, y1=None, dtype=np.float32):
    """(a, direction, boundary): a [H, W] in `dtype`, the share of every pixel that its neighbour takes (0: the pixel is
    copied); direction int8 [H, W], the index into DIRECTIONS of that neighbour (-1: none); boundary bool [H, W], the
    pixels with a differing neighbour."""
    d_ = dtype
    tri = np.ascontiguousarray(tri, np.float32)
    H, W = np.asarray(winner).shape
    T = tri.shape[0]
    y1 = H if y1 is None else y1
    a = np.zeros((H, W), d_)
    direction = np.full((H, W), -1, np.int8)
    boundary = np.zeros((H, W), bool)
    if T == 0:
        return a, direction, boundary
    own = validated(winner, T, pos_of, y0, y1)
    proj = tex_ref.project(tri, P, W, H).astype(d_)
    where = np.arange(T) if pos_of is None else np.asarray(pos_of).astype(np.int64)
    bits = np.full(T, 7, np.uint8) if edges is None else np.asarray(edges, np.uint8)
    zp = np.asarray(z, np.float32)
    half = d_(0.5)
    with np.errstate(all="ignore"):
        for k, (dx, dy) in enumerate(DIRECTIONS):
            ys, xs = np.mgrid[y0:y1, 0:W]
            qx, qy = xs + dx, ys + dy
            ok = (qx >= 0) & (qx < W) & (qy >= y0) & (qy < y1)          # a strip does not see across its edge
            ys, xs, qx, qy = ys[ok], xs[ok], qx[ok], qy[ok]
            wp, wq = own[ys, xs], own[qy, qx]
            sel = wp != wq
            ys, xs, qx, qy, wp, wq = ys[sel], xs[sel], qx[sel], qy[sel], wp[sel], wq[sel]
            if not len(ys):
                continue
            boundary[ys, xs] = True
            near_is_q = (wq >= 0) & ((wp < 0) | (zp[qy, qx] < zp[ys, xs]))      # (a NaN makes p the near one)
            w = np.where(near_is_q, wq, wp)
            nx, ny = np.where(near_is_q, qx, xs), np.where(near_is_q, qy, ys)
            fx, fy = np.where(near_is_q, xs, qx), np.where(near_is_q, ys, qy)
            c = proj[where[w]]
            bn = tex_ref.barycentrics(c, nx, ny)
            bf = tex_ref.barycentrics(c, fx, fy)
            t = np.full(len(w), np.inf, d_)
            ks = np.zeros(len(w), np.int64)
            for j in range(3):
                tk = bn[j] / (bn[j] - bf[j])
                take = (bf[j] < 0) & (tk < t)                                     # (a NaN is never taken)
                t = np.where(take, tk, t)
                ks = np.where(take, j + 1, ks)
            e = ks % 3
            drawn = ((bits[w] >> e) & 1).astype(bool)
            s = np.where(near_is_q, t - half, half - t)
            s = np.where(s > half, half, s)
            cur = a[ys, xs]
            take = (ks > 0) & drawn & (s > cur)                                   # (the first direction wins a tie)
            a[ys[take], xs[take]] = s[take]
            direction[ys[take], xs[take]] = k
    return a, direction, boundary


def edge_aa(color, winner, z, tri, pos_of, P, edges=None, y0=0, y1=None, dtype=np.float32, out=None, counts=None):
    """(out, a, direction): the plane crender_wire_edge_aa writes over rows y0 .. y1 (in `dtype`; the other rows are
    `out`'s, zeros without one, as ``AdvancedPixelBufferFiller.edge_aa`` leaves them), with ``coverage``'s a and
    direction.  `counts`, a dict, receives the number of boundary pixels, of blended ones and the histogram of their a
    in the four bins (0, 1/8], (1/8, 1/4], (1/4, 3/8], (3/8, 1/2]."""
    d_ = dtype
    color = np.asarray(color, np.float32)
    H, W = color.shape[:2]
    y1 = H if y1 is None else y1
    a, direction, boundary = coverage(winner, z, tri, pos_of, P, edges, y0, y1, d_)
    res = np.zeros((H, W, 3), d_) if out is None else np.array(out, copy=True).astype(d_)
    res[y0:y1] = color[y0:y1].astype(d_)
    ys, xs = np.nonzero(a != 0)
    if len(ys):
        k = direction[ys, xs]
        step = np.asarray(DIRECTIONS)[k]
        av = a[ys, xs][:, None]
        kk = d_(1) - av
        with np.errstate(all="ignore"):
            res[ys, xs] = color[ys, xs].astype(d_) * kk + color[ys + step[:, 1], xs + step[:, 0]].astype(d_) * av
    if counts is not None:
        hit = a[a != 0].astype(np.float64)
        counts.update(boundary=int(boundary.sum()), blended=int(len(hit)),
                      bins=[int(((hit > lo) & (hit <= lo + 0.125)).sum()) for lo in (0.0, 0.125, 0.25, 0.375)])
    return res, a, direction
