"""Host model of normal mapping: the statements of crender_nmap_from_height and crender_nmap_shade
(include/crender_nmap.h) in vectorised numpy, one float32 operation per step, on top of tests/tex_ref.py (the covered
pixels, projection, barycentrics, uv, the nearest and the bilinear sample) and tests/mip_ref.py (the chain, the level of
a footprint, the trilinear sample).  The GPU tests compare csrc/normal_map.hip's k_nmap_* with it bit for bit;
tests/test_normal_map_cpu.py pins it by counts on the oracle's frames, by identities and against itself in float64.

``dtype=np.float64`` evaluates the decode, the tangent frame and the result in double precision from the same float32
barycentrics, uv and samples."""
import numpy as np

import mip_ref
import tex_ref

FLAT = (128, 128, 255)
FILTERS = ("nearest", "bilinear", "trilinear")


def from_height(height, scale=1.0, wrap=False):
    """uint8 [mh, mw, 3]: crender_nmap_from_height of a uint8 [mh, mw] height map."""
    h = np.ascontiguousarray(height, np.uint8).astype(np.int32)
    assert h.ndim == 2 and h.size
    mh, mw = h.shape
    d = np.float32
    r, c = np.arange(mh), np.arange(mw)
    if wrap:
        cl, cr, ru, rd = (c - 1) % mw, (c + 1) % mw, (r - 1) % mh, (r + 1) % mh
    else:
        cl, cr, ru, rd = np.maximum(c - 1, 0), np.minimum(c + 1, mw - 1), np.maximum(r - 1, 0), np.minimum(r + 1, mh - 1)
    with np.errstate(all="ignore"):
        k = d(scale) / d(255.0)
        gx = (h[:, cr] - h[:, cl]).astype(d) * k
        gy = (h[ru, :] - h[rd, :]).astype(d) * k             # v points up: the row above minus the row below
        ln = np.sqrt((gx * gx + gy * gy) + d(1))
        v = np.stack([-gx / ln, -gy / ln, d(1) / ln], axis=2)
        b = np.rint(v * d(127) + d(128))
        b = np.where(~(b > 0), d(0), np.where(b > d(255), d(255), b))       # (a NaN gives 0)
    return b.astype(np.uint8)


def decode(nmap):
    """float64 [.., 3]: the vectors the bytes of a map stand for (before any clamp)."""
    return (np.asarray(nmap, np.float64) - 128.0) / 127.0


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def samples(winner, tri, P, uv, nmap, perspective=True, filter="bilinear", y0=0, y1=None, chain=None):
    """(ys, xs, t, s): the covered pixels of the rows, their winners and their float32 [N, 3] samples of the map."""
    assert filter in FILTERS
    nmap = np.ascontiguousarray(np.asarray(nmap)[:, :, :3], np.uint8)
    mh, mw = nmap.shape[:2]
    tri = np.ascontiguousarray(tri, np.float32)
    if filter == "trilinear":
        chain = mip_ref.build_chain(nmap) if chain is None else chain
        ys, xs, u, v, _, l0, f = mip_ref.pixel_levels(winner, tri, P, uv, mh, mw, perspective, y0, y1)
        t = tex_ref.covered(winner, tri.shape[0], y0, y1)[2]
        return ys, xs, t, mip_ref.trilinear(u, v, l0, f, chain)
    ys, xs, t, u, v = tex_ref.pixel_uv(winner, tri, P, uv, perspective, y0, y1)
    with np.errstate(all="ignore"):
        return ys, xs, t, (tex_ref.bilinear if filter == "bilinear" else tex_ref.nearest)(u, v, nmap)


def normal_map_pass(normals, winner, tri, P, uv, nmap, perspective=True, filter="bilinear", strength=1.0, y0=0, y1=None,
                    counts=None, dtype=np.float32, chain=None):
    """A copy of the normal plane after crender_nmap_shade over rows y0 .. y1 (in `dtype`).  `counts`, a dict, receives
    the number of covered and of written pixels, of those whose triangle has degenerate uv (``det_zero``: neither
    det > 0 nor det < 0), mirrored uv (det < 0) and of those that take the sign change of the bitangent (``flipped``),
    and ``mask``, the [H, W] mask of the written pixels."""
    d_ = dtype
    out = np.array(normals, np.float32, copy=True).astype(d_)
    tri = np.ascontiguousarray(tri, np.float32)
    uv = np.asarray(uv, np.float32)
    y1 = out.shape[0] if y1 is None else y1
    ys, xs, t, s = samples(winner, tri, P, uv, nmap, perspective, filter, y0, y1, chain)
    with np.errstate(all="ignore"):
        # the decode
        m = (s.astype(d_) - d_(128)) / d_(127)
        m = np.where(m < d_(-1), d_(-1), m)
        st = d_(np.float32(strength))
        mx, my, mz = m[:, 0] * st, m[:, 1] * st, m[:, 2]
        # the tangent frame of the triangle
        c, w = tri[t].astype(d_), uv[t].astype(d_)
        e1 = [c[:, 1, j] - c[:, 0, j] for j in range(3)]
        e2 = [c[:, 2, j] - c[:, 0, j] for j in range(3)]
        du1, dv1 = w[:, 1, 0] - w[:, 0, 0], w[:, 1, 1] - w[:, 0, 1]
        du2, dv2 = w[:, 2, 0] - w[:, 0, 0], w[:, 2, 1] - w[:, 0, 1]
        det = du1 * dv2 - du2 * dv1
        sg = np.where(det < 0, d_(-1), d_(1))
        Tt = [(e1[j] * dv2 - e2[j] * dv1) * sg for j in range(3)]
        Bt = [(e2[j] * du1 - e1[j] * du2) * sg for j in range(3)]
        # the frame around the stored normal
        n = [np.asarray(normals, np.float32)[ys, xs, j].astype(d_) for j in range(3)]
        nl = np.sqrt(_dot(n, n))
        Nu = [n[j] / nl for j in range(3)]
        d = _dot(Nu, Tt)
        Tp = [Tt[j] - Nu[j] * d for j in range(3)]
        tl = np.sqrt(_dot(Tp, Tp))
        Tu = [Tp[j] / tl for j in range(3)]
        Bp = [Nu[1] * Tu[2] - Nu[2] * Tu[1], Nu[2] * Tu[0] - Nu[0] * Tu[2], Nu[0] * Tu[1] - Nu[1] * Tu[0]]
        flip = _dot(Bp, Bt) < 0
        Bp = [np.where(flip, -Bp[j], Bp[j]) for j in range(3)]
        res = np.stack([(Tu[j] * mx + Bp[j] * my) + Nu[j] * mz for j in range(3)], axis=1)
        write = ((det > 0) | (det < 0)) & (nl > 0) & (tl > 0) & ((mx < 0) | (mx > 0) | (my < 0) | (my > 0))
    out[ys[write], xs[write]] = res[write]
    if counts is not None:
        mask = np.zeros(out.shape[:2], bool)
        mask[ys[write], xs[write]] = True
        counts.update(covered=len(t), written=int(write.sum()), det_zero=int((~((det > 0) | (det < 0))).sum()),
                      mirrored=int((det < 0).sum()), flipped=int(flip.sum()), mask=mask)
    return out
