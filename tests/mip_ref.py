"""Host model of the mip chain and the trilinear texture pass: the statements of include/crender_mip.h in
vectorised numpy, one float32 operation per step, on top of tests/tex_ref.py (projection, barycentrics, uv and
the bilinear sample are its own).  The GPU tests compare csrc/texmip.hip with it bit for bit;
tests/test_mipmap_cpu.py pins it on hand-made chains, known footprints and the T-Rex level histograms."""
import numpy as np

import tex_ref

MAX_LEVELS = 16


def layout(th, tw):
    """(levels [(h_k, w_k)], byte offsets, total bytes) of the chain of a th x tw texture."""
    if th < 1 or tw < 1:
        raise ValueError("a texture has at least one texel")
    L = 1 + int(max(th, tw)).bit_length() - 1          # 1 + floor(log2(max side))
    if L > MAX_LEVELS:
        raise ValueError("more than 16 levels")
    levels, offsets, at = [], [], 0
    h, w = th, tw
    for _ in range(L):
        levels.append((h, w))
        offsets.append(at)
        at += 3 * h * w
        h, w = max(1, h >> 1), max(1, w >> 1)
    return levels, offsets, at


def reduce_level(prev):
    """Level k from level k - 1: (A + B + C + D + 2) >> 2 over the edge-clamped 2 x 2 block, in integers."""
    h, w = prev.shape[:2]
    hk, wk = max(1, h >> 1), max(1, w >> 1)
    r, c = np.arange(hk), np.arange(wk)
    r0, r1 = np.minimum(2 * r, h - 1), np.minimum(2 * r + 1, h - 1)
    c0, c1 = np.minimum(2 * c, w - 1), np.minimum(2 * c + 1, w - 1)
    p = prev[:, :, :3].astype(np.uint32)
    s = p[r0][:, c0] + p[r0][:, c1] + p[r1][:, c0] + p[r1][:, c1] + 2
    return (s >> 2).astype(np.uint8)


def build_chain(tex):
    """The list of levels, uint8 [h_k, w_k, 3]; level 0 is the texture."""
    tex = np.ascontiguousarray(np.asarray(tex)[:, :, :3], dtype=np.uint8)
    levels, _, _ = layout(*tex.shape[:2])
    chain = [tex]
    for _ in levels[1:]:
        chain.append(reduce_level(chain[-1]))
    assert [c.shape[:2] for c in chain] == levels
    return chain


def pack_chain(chain):
    """The chain as the device holds it: levels packed tightly in order."""
    return np.concatenate([c.reshape(-1) for c in chain])


def footprint(u, v, ux, vx, uy, vy, th, tw):
    """rho of the statement: the longer of the two texel-space steps per pixel."""
    d = np.float32
    with np.errstate(all="ignore"):
        dudx, dvdx = (ux - u) * d(tw), (vx - v) * d(th)
        dudy, dvdy = (uy - u) * d(tw), (vy - v) * d(th)
        rx = dudx * dudx + dvdx * dvdx
        ry = dudy * dudy + dvdy * dvdy
        r2 = np.where(rx >= ry, rx, ry)            # a NaN rx gives ry, a NaN ry gives NaN
        return np.sqrt(r2)


def level_and_weight(rho, L):
    """(l0 int32, f float32) by comparisons and one exact scaling: no log2."""
    rho = np.asarray(rho, np.float32)
    l0 = np.zeros(rho.shape, np.int32)
    f = np.zeros(rho.shape, np.float32)
    with np.errstate(all="ignore"):
        minified = rho > np.float32(1)
        top = minified & ~(rho < np.float32(2.0 ** (L - 1)))
        mid = minified & ~top
    l0[top] = L - 1
    m, e1 = np.frexp(rho[mid])                      # rho = m * 2^e1 with 0.5 <= m < 1
    e = e1.astype(np.int32) - 1
    l0[mid] = e
    f[mid] = np.ldexp(rho[mid], -e).astype(np.float32) - np.float32(1)
    return l0, f


def pixel_levels(winner, tri, P, uv, th, tw, perspective=False, y0=0, y1=None):
    """(ys, xs, u, v, rho, l0, f) of the covered pixels of the rows."""
    tri = np.ascontiguousarray(tri, np.float32)
    H, W = winner.shape
    ys, xs, t = tex_ref.covered(winner, tri.shape[0], y0, y1)
    proj = tex_ref.project(tri, P, W, H)[t]
    uv_t, z_t = np.asarray(uv, np.float32)[t], tri[:, :, 2][t]
    L = len(layout(th, tw)[0])
    with np.errstate(all="ignore"):
        u, v = tex_ref.uv_at(uv_t, z_t, *tex_ref.barycentrics(proj, xs, ys), perspective)
        ux, vx = tex_ref.uv_at(uv_t, z_t, *tex_ref.barycentrics(proj, xs + 1, ys), perspective)
        uy, vy = tex_ref.uv_at(uv_t, z_t, *tex_ref.barycentrics(proj, xs, ys + 1), perspective)
    rho = footprint(u, v, ux, vx, uy, vy, th, tw)
    l0, f = level_and_weight(rho, L)
    return ys, xs, u, v, rho, l0, f


def trilinear(u, v, l0, f, chain):
    """Colour of each pixel: bilinear on level l0, blended with level l0 + 1 where f != 0."""
    out = np.zeros((len(u), 3), np.float32)
    with np.errstate(all="ignore"):
        for k, level in enumerate(chain):
            at = l0 == k
            if at.any():
                out[at] = tex_ref.bilinear(u[at], v[at], level)
            up = (l0 == k - 1) & (f != 0)
            if k and up.any():
                a, w = out[up], f[up][:, None]
                b = tex_ref.bilinear(u[up], v[up], level)
                out[up] = a * (np.float32(1) - w) + b * w
    return out


def texture_pass(color, winner, tri, P, uv, tex, perspective=False, normals=None, light_direction=None, y0=0,
                 y1=None, chain=None):
    """A copy of `color` after crender_mip_shade over rows y0 .. y1 (tex_ref.texture_pass's arguments)."""
    out = np.array(color, np.float32, copy=True)
    y1 = out.shape[0] if y1 is None else y1
    chain = build_chain(tex) if chain is None else chain
    th, tw = chain[0].shape[:2]
    ys, xs, u, v, _, l0, f = pixel_levels(winner, tri, P, uv, th, tw, perspective, y0, y1)
    out[ys, xs] = trilinear(u, v, l0, f, chain)
    if light_direction is not None:
        from oracle import oracle as O
        rows = np.ascontiguousarray(out[y0:y1])
        O.guro(rows, np.ascontiguousarray(normals[y0:y1]), light_direction)
        out[y0:y1] = rows
    return out
