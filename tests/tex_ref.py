"""Host model of the deferred texture pass: the statements of include/crender_tex.h in vectorised
numpy, one float32 operation per step, over (winner plane, unprojected triangles, projection matrix,
uv, texture, flags, light).  The GPU tests compare csrc/texture.hip with it bit for bit;
tests/test_texture_cpu.py pins it on the oracle's colour plane, ``oracle.bar`` and ``Model``'s texel rule.

``dtype=np.float64`` evaluates the same statements in double precision from the same float32 inputs (the
projection included): the yardstick of the perspective statement's rounding."""
import numpy as np

INT_MIN = np.int32(-2147483648)


def project(tri, P, w, h, dtype=np.float32):
    """crender_project (.pyx:116-130); float32 goes through the oracle's C restatement."""
    if dtype == np.float32:
        from oracle import oracle as O
        return O.project(tri, P, w, h)
    v = np.asarray(tri, np.float32).astype(dtype).copy()
    P = np.asarray(P, np.float32).astype(dtype)
    z = v[..., 2].copy()
    for j in range(3):          # in place: column j sees the columns before it already overwritten
        v[..., j] = v[..., 0] * P[0, j] + v[..., 1] * P[1, j] + v[..., 2] * P[2, j] + P[3, j]
    for j in range(3):
        v[..., j] = v[..., j] / z
    v[..., 0] = (v[..., 0] + 1) * dtype(w / 2.0)
    v[..., 1] = (v[..., 1] + 1) * dtype(h / 2.0)
    return v


def covered(winner, T, y0=0, y1=None):
    """(ys, xs, t) of the pixels of rows y0 .. y1 whose winner is a triangle."""
    y1 = winner.shape[0] if y1 is None else y1
    rows = winner[y0:y1]
    ys, xs = np.nonzero((rows >= 0) & (rows < T))
    return ys + y0, xs, rows[ys, xs].astype(np.int64)


def barycentrics(proj, xs, ys):
    """math_utils.pyx:8-34 at integer pixels; proj: [N, 3, 3] projected triangles, one per pixel."""
    d = proj.dtype.type
    x0, y0, x1, y1, x2, y2 = proj[:, 0, 0], proj[:, 0, 1], proj[:, 1, 0], proj[:, 1, 1], proj[:, 2, 0], proj[:, 2, 1]
    fx, fy = xs.astype(d), ys.astype(d)
    l01, l02 = x1 - x2, y1 - y2
    l03 = l01 * (y0 - y2) - l02 * (x0 - x2)
    l11, l12 = x2 - x0, y2 - y0
    l13 = l11 * (y1 - y0) - l12 * (x1 - x0)
    l21, l22 = x0 - x1, y0 - y1
    l23 = l21 * (y2 - y1) - l22 * (x2 - x1)
    b1 = (l01 * (fy - y2) - l02 * (fx - x2)) / l03
    b2 = (l11 * (fy - y0) - l12 * (fx - x0)) / l13
    b3 = (l21 * (fy - y1) - l22 * (fx - x1)) / l23
    return b1, b2, b3


def interp(a0, a1, a2, b1, b2, b3):
    return a0 * b1 + a1 * b2 + a2 * b3


def uv_at(uv_t, z_t, b1, b2, b3, perspective):
    """(u, v) of each pixel; uv_t [N, 3, 2], z_t [N, 3] the unprojected z of the corners."""
    if not perspective:
        return (interp(uv_t[:, 0, 0], uv_t[:, 1, 0], uv_t[:, 2, 0], b1, b2, b3),
                interp(uv_t[:, 0, 1], uv_t[:, 1, 1], uv_t[:, 2, 1], b1, b2, b3))
    q1, q2, q3 = b1 / z_t[:, 0], b2 / z_t[:, 1], b3 / z_t[:, 2]
    s = (q1 + q2) + q3
    return (((uv_t[:, 0, 0] * q1 + uv_t[:, 1, 0] * q2) + uv_t[:, 2, 0] * q3) / s,
            ((uv_t[:, 0, 1] * q1 + uv_t[:, 1, 1] * q2) + uv_t[:, 2, 1] * q3) / s)


def host_i32(f):
    """The host's truncating float -> int32 conversion: INT_MIN for a NaN and anything outside int32."""
    f = np.asarray(f)
    out = np.full(f.shape, INT_MIN, np.int32)
    ok = (f >= -2147483648.0) & (f < 2147483648.0)
    out[ok] = np.trunc(f[ok]).astype(np.int32)
    return out


def nearest(u, v, tex):
    th, tw = tex.shape[:2]
    d = u.dtype.type
    row = np.clip(host_i32((d(1) - v) * d(th)), 0, th - 1)
    colm = np.clip(host_i32(u * d(tw)), 0, tw - 1)
    return tex[row, colm, :3].astype(d)


def bilinear(u, v, tex):
    th, tw = tex.shape[:2]
    d = u.dtype.type
    fx, fy = u * d(tw) - d(0.5), (d(1) - v) * d(th) - d(0.5)
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[:, None], (fy - y0)[:, None]
    c0, c1 = np.clip(host_i32(x0), 0, tw - 1), np.clip(host_i32(x0 + d(1)), 0, tw - 1)
    r0, r1 = np.clip(host_i32(y0), 0, th - 1), np.clip(host_i32(y0 + d(1)), 0, th - 1)
    t = tex[:, :, :3]
    t00, t01, t10, t11 = t[r0, c0].astype(d), t[r0, c1].astype(d), t[r1, c0].astype(d), t[r1, c1].astype(d)
    wx, wy = d(1) - ax, d(1) - ay
    return (t00 * wx + t01 * ax) * wy + (t10 * wx + t11 * ax) * ay


def pixel_uv(winner, tri, P, uv, perspective=False, y0=0, y1=None, dtype=np.float32):
    """(ys, xs, t, u, v) of the covered pixels of the rows."""
    tri = np.ascontiguousarray(tri, np.float32)
    H, W = winner.shape
    ys, xs, t = covered(winner, tri.shape[0], y0, y1)
    proj = project(tri, P, W, H, dtype)
    with np.errstate(all="ignore"):
        b1, b2, b3 = barycentrics(proj[t], xs, ys)
        u, v = uv_at(np.asarray(uv, np.float32).astype(dtype)[t], tri[:, :, 2].astype(dtype)[t], b1, b2, b3, perspective)
    return ys, xs, t, u, v


def texture_pass(color, winner, tri, P, uv, tex, perspective=False, bilinear_filter=False, normals=None,
                 light_direction=None, y0=0, y1=None):
    """A copy of `color` after crender_tex_shade over rows y0 .. y1.  `light_direction` is what
    ``GuroIllumination`` is constructed with (``oracle.guro`` flips and normalises it as that class does)."""
    out = np.array(color, np.float32, copy=True)
    y1 = out.shape[0] if y1 is None else y1
    ys, xs, _, u, v = pixel_uv(winner, tri, P, uv, perspective, y0, y1)
    with np.errstate(all="ignore"):
        out[ys, xs] = (bilinear if bilinear_filter else nearest)(u, v, np.asarray(tex))
    if light_direction is not None:
        from oracle import oracle as O
        rows = np.ascontiguousarray(out[y0:y1])
        O.guro(rows, np.ascontiguousarray(normals[y0:y1]), light_direction)
        out[y0:y1] = rows
    return out
