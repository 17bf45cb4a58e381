"""The host model of the motion passes (include/crender_motion.h): the contract's statements in numpy, one array operation
per float32 operation, in the contract's order.  ``motion_vectors`` is built on ``shadow_ref.light_point`` (the blend of
the previous pose's corners) and the oracle's projection; ``motion_blur`` walks the taps of every tile over the whole
frame at once.  The GPU tests compare the kernels with it bit for bit; tests/test_motion_cpu.py pins it by hand and against
its own float64 evaluation (``dtype=np.float64``: the same statements from the same float32 inputs, every intermediate in
double)."""
import numpy as np

import shadow_ref
import tex_ref

MAX_RADIUS, MAX_TAPS, TILE = 12, 32, 32
FAR = np.float32(3.40282346638528859812e+38)


def _project_points(X, Y, Z, P, W, H, dtype):
    pts = np.stack([X, Y, Z], 1).reshape(-1, 1, 3)
    if not len(pts):
        return np.zeros((0, 3), dtype)
    if dtype == np.float32:
        return tex_ref.project(np.ascontiguousarray(pts.repeat(3, 1), np.float32), P, W, H)[:, 0]
    v = pts.astype(dtype).copy()
    Pm = np.asarray(P, np.float32).astype(dtype)
    z = v[..., 2].copy()
    for j in range(3):
        v[..., j] = v[..., 0] * Pm[0, j] + v[..., 1] * Pm[1, j] + v[..., 2] * Pm[2, j] + Pm[3, j]
    for j in range(3):
        v[..., j] = v[..., j] / z
    v[..., 0] = (v[..., 0] + 1) * dtype(np.float32(W / 2.0))
    v[..., 1] = (v[..., 1] + 1) * dtype(np.float32(H / 2.0))
    return v[:, 0]


def _prev_point64(winner, tri, P, prev, y0, y1):
    """shadow_ref.light_point's statements in float64 from the same float32 inputs."""
    d = np.float64
    H, W = winner.shape
    ys, xs, t = tex_ref.covered(winner, tri.shape[0], y0, y1)
    proj = tex_ref.project(tri, P, W, H, d)
    with np.errstate(all="ignore"):
        b1, b2, b3 = tex_ref.barycentrics(proj[t], xs, ys)
        z = tri[:, :, 2].astype(d)[t]
        q1, q2, q3 = b1 / z[:, 0], b2 / z[:, 1], b3 / z[:, 2]
        s = (q1 + q2) + q3
        c = prev.astype(d)[t]
        X, Y, Z = (((c[:, 0, k] * q1 + c[:, 1, k] * q2) + c[:, 2, k] * q3) / s for k in range(3))
    return ys, xs, t, X, Y, Z


def motion_vectors(winner, tri, P, prev_tri, exposure=1.0, y0=0, y1=None, out=None, dtype=np.float32):
    """The plane crender_motion_vectors leaves: `out` (zeros without one) with the rows y0 .. y1 written."""
    d = dtype
    winner = np.asarray(winner, np.int32)
    tri, prev = np.ascontiguousarray(tri, np.float32), np.ascontiguousarray(prev_tri, np.float32)
    H, W = winner.shape
    y1 = H if y1 is None else y1
    res = np.zeros((H, W, 2), d) if out is None else np.array(out, d)
    res[y0:y1] = 0
    if tri.shape[0] == 0:
        return res
    if d == np.float32:
        ys, xs, t, X, Y, Z = shadow_ref.light_point(winner, tri, P, prev, y0, y1)
    else:
        ys, xs, t, X, Y, Z = _prev_point64(winner, tri, P, prev, y0, y1)
    with np.errstate(all="ignore"):
        p = _project_points(X, Y, Z, P, W, H, d)
        e = d(np.float32(exposure))
        vx = (xs.astype(d) - p[:, 0]) * e
        vy = (ys.astype(d) - p[:, 1]) * e
        ok = (Z > 0) & np.isfinite(vx) & np.isfinite(vy)
    res[ys[ok], xs[ok], 0] = vx[ok]
    res[ys[ok], xs[ok], 1] = vy[ok]
    return res


def view_depth(P, z, dtype=np.float32):
    P16 = np.asarray(P, np.float32).reshape(16)
    with np.errstate(all="ignore"):
        return dtype(P16[14]) / (np.asarray(z, np.float32).astype(dtype) - dtype(P16[10]))


def half_velocity(velocity, max_radius, dtype=np.float32):
    """(hx, hy, l) of every pixel: the half velocity clamped to max_radius and its length."""
    d = dtype
    v = np.asarray(velocity, np.float32).astype(d)
    Rf = d(max_radius)
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(v[..., 0]) & np.isfinite(v[..., 1]))
        vx, vy = np.where(bad, d(0), v[..., 0]), np.where(bad, d(0), v[..., 1])
        hx, hy = vx * d(0.5), vy * d(0.5)
        l = np.sqrt(hx * hx + hy * hy)
        over = l > Rf
        k = Rf / np.where(over, l, d(1))
        hx, hy = np.where(over, hx * k, hx), np.where(over, hy * k, hy)
        l = np.where(over, Rf, l)
    return hx.astype(d), hy.astype(d), l.astype(d)


def tile_taps(Dx, Dy, taps, max_radius, dtype=np.float32):
    """(ox, oy, dist) of the taps of dominant half velocities Dx, Dy (arrays): int [taps, ...] twice and dtype [taps, ...]."""
    d = dtype
    i = np.arange(taps)
    tau = ((2 * i + 1 - taps).astype(d) / d(taps)).reshape((taps,) + (1,) * np.ndim(Dx))
    ox = np.clip(np.rint(np.asarray(Dx, d)[None] * tau).astype(np.int64), -max_radius, max_radius)
    oy = np.clip(np.rint(np.asarray(Dy, d)[None] * tau).astype(np.int64), -max_radius, max_radius)
    return ox, oy, np.sqrt((ox * ox + oy * oy).astype(np.float32).astype(d))


def _clamp01(a):
    return np.where(a < 0, a.dtype.type(0), np.where(a > 1, a.dtype.type(1), a))


def _cone(m):
    t = m.dtype.type(1) - m
    return np.where(t > 0, t, m.dtype.type(0))


def _cyl(m):
    d = m.dtype.type
    u = _clamp01((m - d(np.float32(0.95))) * d(10))
    return d(1) - (u * u) * (d(3) - d(2) * u)


def motion_blur(color, winner, z, T, P, velocity, max_radius=8, taps=16, soft=0.02, y0=0, y1=None, out=None, counts=None,
                dtype=np.float32, mask=None, dominant=None):
    """The plane crender_motion_blur leaves: `out` (zeros without one) with the rows y0 .. y1 written.  `counts`, a dict,
    receives covered (pixels of the rows with a winner in [0, T)), moving (pixels of the rows with l > 1/2), tiles_copied,
    copied and blurred (pixels of the rows), taps_taken and largest_l; `mask`, a bool plane, receives which pixels are
    blurred; `dominant`, a list, receives (tile x0, tile y0, x, y) of every tile's dominant pixel."""
    d = dtype
    color = np.ascontiguousarray(color, np.float32)
    winner = np.asarray(winner, np.int32)
    H, W = winner.shape
    y1 = H if y1 is None else y1
    R, N = int(max_radius), int(taps)
    assert 1 <= R <= MAX_RADIUS and 1 <= N <= MAX_TAPS and color.shape == (H, W, 3) and np.shape(velocity) == (H, W, 2)
    isoft = d(1) / d(np.float32(soft))
    hx, hy, l = half_velocity(velocity, R, d)
    covered = (winner >= 0) & (winner.astype(np.int64) < T)
    with np.errstate(all="ignore"):
        il = d(1) / np.where(l > d(0.5), l, d(0.5))
        zv = np.where(covered, view_depth(P, z, d), d(FAR)).astype(d)
    # ---- the dominant pixel of every tile, and the tile's taps
    nty, ntx = (y1 - y0 + TILE - 1) // TILE, (W + TILE - 1) // TILE
    Dx, Dy, walk = np.zeros((nty, ntx), d), np.zeros((nty, ntx), d), np.zeros((nty, ntx), bool)
    for ty in range(nty):
        r0, r1 = max(y0, y0 + ty * TILE - R), min(y1, y0 + (ty + 1) * TILE + R)
        for tx in range(ntx):
            c0, c1 = max(0, tx * TILE - R), min(W, (tx + 1) * TILE + R)
            window = l[r0:r1, c0:c1]
            at = int(np.argmax(window))              # the first of equals in row-major order, which is the frame's
            yy, xx = r0 + at // (c1 - c0), c0 + at % (c1 - c0)
            Dx[ty, tx], Dy[ty, tx], walk[ty, tx] = hx[yy, xx], hy[yy, xx], l[yy, xx] > d(0.5)
            if dominant is not None:
                dominant.append((tx * TILE, y0 + ty * TILE, xx, yy))
    ox, oy, dist = tile_taps(Dx, Dy, N, R, d)        # [N, nty, ntx]
    rows, cols = np.arange(y0, y1), np.arange(W)
    tyi, txi = (rows - y0) // TILE, cols // TILE
    yy, xx = np.meshgrid(rows, cols, indexing="ij")
    il_p, zv_p, col = il[y0:y1], zv[y0:y1], color.astype(d)
    walk_p = walk[np.ix_(tyi, txi)]
    Sw = il_p.copy()
    S = col[y0:y1] * il_p[..., None]
    any_tap = np.zeros(il_p.shape, bool)
    taken = 0
    with np.errstate(all="ignore"):
        for i in range(N):
            oxp, oyp, dp = ox[i][np.ix_(tyi, txi)], oy[i][np.ix_(tyi, txi)], dist[i][np.ix_(tyi, txi)]
            qy, qx = yy + oyp, xx + oxp
            ok = walk_p & ((oxp != 0) | (oyp != 0)) & (qy >= y0) & (qy < y1) & (qx >= 0) & (qx < W)
            qy, qx = np.where(ok, qy, y0), np.where(ok, qx, 0)
            il_q, zv_q = il[qy, qx], zv[qy, qx]
            mq, mp = dp * il_q, dp * il_p
            fg = _clamp01(d(1) - (zv_q - zv_p) * isoft)
            bg = _clamp01(d(1) - (zv_p - zv_q) * isoft)
            alpha = (fg * _cone(mq) + bg * _cone(mp)) + d(2) * (_cyl(mq) * _cyl(mp))
            take = ok & (alpha > 0)
            if not take.any():
                continue
            Sw = np.where(take, Sw + alpha, Sw)
            S = np.where(take[..., None], S + alpha[..., None] * col[qy, qx], S)
            any_tap |= take
            taken += int(take.sum())
        result = np.where(any_tap[..., None], S / Sw[..., None], col[y0:y1])
    res = np.zeros((H, W, 3), d) if out is None else np.array(out, d)
    if d is np.float32:
        # the copied pixels keep their bits (np.where above may quiet a signalling NaN on some hosts)
        result = np.ascontiguousarray(result, np.float32)
        keep = ~any_tap
        result.view(np.uint32)[keep] = color[y0:y1].view(np.uint32)[keep]
    res[y0:y1] = result
    if counts is not None:
        counts.update(covered=int(covered[y0:y1].sum()), moving=int((l[y0:y1] > d(0.5)).sum()),
                      tiles_copied=int((~walk).sum()), copied=int((~any_tap).sum()), blurred=int(any_tap.sum()),
                      taps_taken=taken, largest_l=float(l[y0:y1].max()))
    if mask is not None:
        mask[...] = False
        mask[y0:y1] = any_tap
    return res


def rotated(tri, angles):
    """The corners `tri` rotated by `angles` (degrees about x, y, z) around their float32 mean: float32 [T, 3, 3], the
    previous pose of the GPU tests (``shadow_ref.rotation_frame`` gives the frame)."""
    Rm, t = shadow_ref.rotation_frame(tri, angles)
    tri = np.asarray(tri, np.float32)
    return np.ascontiguousarray((tri.reshape(-1, 3) @ Rm.T + t).reshape(tri.shape).astype(np.float32))
