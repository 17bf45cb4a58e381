"""Vectorised host model of the numpy filler's whole-sequence draw (include/crender_py.h), independent
of any BLAS: the fma of the contract is emulated exactly (Boldo & Melquiond's fma through a
round-to-odd sum), the sequential depth rule is the key rule of the header.  Pinned to the reference's
fixtures in tests/test_pyrender_cpu.py; the GPU tests compare the device planes with it."""
import numpy as np

TIE_MAX = 0x7FFFFFFF


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _round_odd_sum(a, b):
    s, e = _two_sum(a, b)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s)


def fma(a, b, c):
    """Correctly rounded a*b + c for float64 a and float32-valued b (b has 24 significant bits)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    t = a * 134217729.0                        # Veltkamp split of a: 27 + 26 bits
    hi = t - (t - a)
    lo = a - hi
    uh, ul = _two_sum(hi * b, lo * b)          # both products exact: a*b = uh + ul
    th, tl = _two_sum(c, uh)
    with np.errstate(invalid="ignore"):
        out = th + _round_odd_sum(tl, ul)
    return np.where(np.isfinite(out), out, a * b + c)


def ordered(f):
    u = np.asarray(f, np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(np.asarray(f) == 0, np.uint64(0), u)
    neg = (u & np.uint64(0x80000000)) != 0
    out = np.where(neg, (~u) & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return np.where(np.isnan(f), np.uint64(0), out)


def project(tri, h, w, fov, z_near=0.1, z_far=1000):
    f = 1 / np.tan(fov / 2 / 180 * np.pi)
    q = z_far / (z_far - z_near)
    P00, P11, P22, P32 = np.array([f / (h / w), f, q, -z_near * q], np.float32)
    x, y, z = tri[..., 0], tri[..., 1], tri[..., 2]
    with np.errstate(all="ignore"):
        px = (x * P00 / z + np.float32(1)) * np.float32(w / 2)
        py = (y * P11 / z + np.float32(1)) * np.float32(h / 2)
        pz = (z * P22 + P32) / z
    return px, py, pz


def _i32(v):
    ok = (v >= -2147483648.0) & (v < 2147483648.0)
    return np.where(ok, np.nan_to_num(v), -2147483648).astype(np.int64)


def _u8(v):
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    return (np.where(ok, np.trunc(np.nan_to_num(v)), 0).astype(np.int64) & 0xFF).astype(np.uint8)


def draw(tri, col, nrm, z_plane, color_plane, n_plane, fov, chunk=4096):
    """Draw [T, 3, 3] triangles in array order onto the planes (z float32 [h, w, 1], colour uint8
    [h, w, 3], normals float32 [h, w, 3]), in place."""
    h, w = z_plane.shape[:2]
    tri = np.asarray(tri, np.float32)
    col = np.asarray(col).astype(np.float64)
    nrm = np.asarray(nrm, np.float32)
    T = len(tri)
    with np.errstate(all="ignore"):
        a = tri[:, 1, :2] - tri[:, 0, :2]
        b = tri[:, 2, :2] - tri[:, 0, :2]
        cross = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        s = (nrm[:, 0] + nrm[:, 1]) + nrm[:, 2]
        culled = (cross == 0) | (np.isfinite(s[:, 0]) & np.isfinite(s[:, 1]) & (s[:, 2] / np.float32(3) >= 0))
        px, py, pz = project(tri, h, w, fov)
        nanx, nany = np.isnan(px).any(1), np.isnan(py).any(1)
        xl = np.clip(_i32(np.where(nanx, np.nan, np.ceil(px.min(1)))), 0, w)
        xr = np.clip(_i32(np.where(nanx, np.nan, np.ceil(px.max(1)))), 0, w)
        yb = np.clip(_i32(np.where(nany, np.nan, np.ceil(py.min(1)))), 0, h)
        yt = np.clip(_i32(np.where(nany, np.nan, np.ceil(py.max(1)))), 0, h)
        bw = np.where(culled, 0, np.maximum(xr - xl, 0))
        bh = np.where(bw > 0, np.maximum(yt - yb, 0), 0)
        bw = np.where(bh > 0, bw, 0)
    key = ordered(z_plane[..., 0].reshape(-1)) << np.uint64(32) | np.uint64(1 << 31)
    nsat = np.zeros(T, np.int64)
    for c0 in range(0, T, chunk):
        ids = np.arange(c0, min(T, c0 + chunk))
        n = (bw[ids] * bh[ids]).astype(np.int64)
        t = np.repeat(ids, n)
        if len(t) == 0:
            continue
        q = np.arange(len(t)) - np.repeat(np.cumsum(n) - n, n)
        x, y = xl[t] + q % bw[t], yb[t] + q // bw[t]
        lam = bary(px[t], py[t], x, y)
        inside = (lam[0] >= 0) & (lam[1] >= 0) & (lam[2] >= 0)
        t, x, y, lam = t[inside], x[inside], y[inside], [v[inside] for v in lam]
        counts = np.bincount(t - c0, minlength=len(ids))
        nsat[ids] = np.minimum(counts, 2)
        cnt = counts[t - c0]
        z = depth(pz[t], cnt, lam)
        ok = (z >= 0) & (z <= 1)
        t, x, y, z = t[ok], x[ok], y[ok], z[ok]
        zf = z.astype(np.float32)
        rank = (t + 1).astype(np.uint64)
        cls0 = z < zf.astype(np.float64)
        k = ordered(zf) << np.uint64(32) | np.where(cls0, np.uint64(TIE_MAX) - rank, np.uint64(1 << 31) | rank)
        pix = y * w + x
        np.minimum.at(key, pix, k)
    low = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
    rank = np.where(low >> 31, low & TIE_MAX, TIE_MAX - (low & TIE_MAX))
    pix = np.nonzero(rank)[0]
    t = rank[pix] - 1
    y, x = pix // w, pix % w
    lam = bary(px[t], py[t], x, y)
    z = depth(pz[t], nsat[t], lam)
    zp, cp, np_ = z_plane.reshape(-1), color_plane.reshape(-1, 3), n_plane.reshape(-1, 3)
    zp[pix] = z.astype(np.float32)
    for c in range(3):
        cp[pix, c] = _u8(interp(lam, col[t, :, c]))
        np_[pix, c] = interp(lam, nrm[t, :, c]).astype(np.float32)


def bary(px, py, x, y):
    X, Y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = []
    with np.errstate(all="ignore"):
        for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            ax, ay = px[:, j] - px[:, k], py[:, j] - py[:, k]
            den = ax * (py[:, i] - py[:, k]) - ay * (px[:, i] - px[:, k])
            num = ax.astype(np.float64) * (Y - py[:, k]) - ay.astype(np.float64) * (X - px[:, k])
            out.append(num / den.astype(np.float64))
    return out


def depth(pz, cnt, lam):
    l0, l1, l2 = lam
    z0, z1, z2 = (pz[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        many = fma(l2, z2, fma(l0, z0, l1 * z1))
        one = fma(l2, z2, fma(l1, z1, l0 * z0))
    return np.where(cnt >= 2, many, one)


def interp(lam, v):
    l0, l1, l2 = lam
    with np.errstate(all="ignore"):
        return fma(l2, v[:, 2], fma(l1, v[:, 1], l0 * v[:, 0]))


def new_planes(h, w):
    return (np.full((h, w, 1), 1e6, np.float32), np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32))
