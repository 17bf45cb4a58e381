"""Host model of the deferred ambient-occlusion pass: the statements of include/crender_ao.h in vectorised numpy, one
float32 operation per step, over (the colour, z and winner planes, the unprojected triangles and the projection matrix,
the normal plane, the tap table).  The GPU tests compare csrc/ao.hip with it bit for bit; tests/test_ao_cpu.py pins it on
hand-built frames, on the oracle's frame of T-Rex by counts, by identities and against itself in float64.

The model follows the contract's words, not the kernel's: an uncovered tap gives ``+0`` through a mask, where the
kernel stages a NaN.  That the two agree is what the bit comparisons show.

``dtype=np.float64`` evaluates the same statements in double precision from the same float32 planes."""
import numpy as np

MAX_TAPS = 64
MAX_RADIUS_PX = 32


def constants(P, W, H, radius, n_taps, dtype=np.float32):
    """(xs, ys, kx, ky, r2, inv_r2, inv_n, p10, p14) of a call: the header's "Constants"."""
    d = dtype
    P = np.asarray(P, np.float32).reshape(16)
    xs, ys = np.float32(W / 2.0), np.float32(H / 2.0)
    rad = np.float32(radius)
    with np.errstate(all="ignore"):        # (a huge or a tiny radius: r2 and inv_r2 overflow to inf or fall to 0)
        kx = d(1.0 / (float(xs) * float(P[0])))
        ky = d(1.0 / (float(ys) * float(P[5])))
        r2 = d(rad) * d(rad)
        inv_r2 = d(1.0 / (float(rad) * float(rad)))
        inv_n = d(1.0 / n_taps)
    return d(xs), d(ys), kx, ky, r2, inv_r2, inv_n, d(P[10]), d(P[14])


def rotated(taps, xs, ys, rotate):
    """[n][N] arrays (dx, dy) of every tap at every pixel: the quarter turn r = (x & 1) | (y & 1) << 1."""
    taps = np.asarray(taps, np.int64).reshape(-1, 2)
    dx = np.broadcast_to(taps[:, 0:1], (len(taps), len(xs)))
    dy = np.broadcast_to(taps[:, 1:2], (len(taps), len(xs)))
    if not rotate:
        return dx, dy
    r = ((xs & 1) | ((ys & 1) << 1))[None, :]
    rdx = np.where(r == 0, dx, np.where(r == 1, -dy, np.where(r == 2, dy, -dx)))
    rdy = np.where(r == 0, dy, np.where(r == 1, dx, np.where(r == 2, -dx, -dy)))
    return rdx, rdy


def face_normals(tri_t, Pp):
    """The FACE_NORMALS statement: g = e1 x e2 of the corners [N, 3, 3], turned to face the eye."""
    A, B, C = tri_t[:, 0], tri_t[:, 1], tri_t[:, 2]
    e1 = [B[:, c] - A[:, c] for c in range(3)]
    e2 = [C[:, c] - A[:, c] for c in range(3)]
    g = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    s = (g[0] * Pp[0] + g[1] * Pp[1]) + g[2] * Pp[2]
    return [np.where(s > 0, -v, v) for v in g]


def ao_pass(color, z, winner, tri, P, normals, taps, radius=0.03, radius_px=8, min_cos=0.1, strength=2.0, floor=0.0,
            rotate=True, face=False, pos_of=None, T=None, y0=0, y1=None, counts=None, dtype=np.float32):
    """A copy of `color` after crender_ao_shade over rows y0 .. y1 (in `dtype`).  `normals` is the normal plane (not
    read with `face`), `taps` the table of (dx, dy).  `counts`, a dict, receives the number of covered pixels, of
    occluded ones (S > 0: the pixels written), of taps taken, of pixels at the floor, the smallest factor and S."""
    d = dtype
    taps = np.asarray(taps, np.int64).reshape(-1, 2)
    n = len(taps)
    assert 1 <= n <= MAX_TAPS and 1 <= radius_px <= MAX_RADIUS_PX
    assert (np.abs(taps) <= radius_px).all() and (taps != 0).any(1).all()
    winner = np.asarray(winner, np.int32)
    H, W = winner.shape
    y1 = H if y1 is None else y1
    T = (0 if tri is None else len(tri)) if T is None else T
    out = np.array(color, np.float32, copy=True).astype(d)
    xs_, ys_, kx, ky, r2, inv_r2, inv_n, p10, p14 = constants(P, W, H, radius, n, d)
    cov = (winner >= 0) & (winner < T)
    cov[:y0] = False
    cov[y1:] = False
    ys, xs = np.nonzero(cov)
    n_covered = len(ys)
    with np.errstate(all="ignore"):
        zv = p14 / (np.asarray(z, np.float32).astype(d) - p10)

        def Q(qx, qy):
            zq = zv[qy, qx]
            return [((qx.astype(d) - xs_) * kx) * zq, ((qy.astype(d) - ys_) * ky) * zq, zq]
        if face:
            t = winner[ys, xs].astype(np.int64)
            if pos_of is not None:
                t = np.asarray(pos_of).astype(np.uint32).astype(np.int64)[t]
            keep = t < T
            ys, xs, t = ys[keep], xs[keep], t[keep]
        Pp = Q(xs, ys)
        if face:
            nrm = face_normals(np.asarray(tri, np.float32)[t].astype(d), Pp)
        else:
            nrm = [np.asarray(normals, np.float32)[ys, xs, c].astype(d) for c in range(3)]
        ln = np.sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]) + d(np.float32(1e-6))
        nu = [v / ln for v in nrm]
        rdx, rdy = rotated(taps, xs, ys, rotate)
        S = np.zeros(len(xs), d)
        taken = 0
        for i in range(n):
            qx, qy = xs + rdx[i], ys + rdy[i]
            on = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            on &= cov[qy, qx]
            q = Q(qx, qy)
            D = [q[c] - Pp[c] for c in range(3)]
            dd = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
            dn = (D[0] * nu[0] + D[1] * nu[1]) + D[2] * nu[2]
            c_ = dn / np.sqrt(dd)
            wgt = d(1) - dd * inv_r2
            take = on & (dd < r2) & (c_ > d(np.float32(min_cos)))
            S = S + np.where(take, c_ * wgt, d(0))
            taken += int(take.sum())
        occ = S > 0
        f = d(1) - d(np.float32(strength)) * (S * inv_n)
        low = f < d(np.float32(floor))
        f = np.where(low, d(np.float32(floor)), f)
        oy, ox = ys[occ], xs[occ]
        out[oy, ox] = out[oy, ox] * f[occ][:, None]
    if counts is not None:
        counts.update(covered=n_covered, occluded=int(occ.sum()), taps_taken=taken,
                      at_floor=int((occ & (f == d(np.float32(floor)))).sum()),
                      min_factor=float(f[occ].min()) if occ.any() else 1.0, S=S, ys=ys, xs=xs)
    return out
