"""Host model of the deferred Phong pass: the statements of include/crender_phong.h in vectorised numpy, one float32
operation per step, over (the winner plane, its unprojected triangles and projection matrix, the normal plane, the
lights).  The GPU tests compare csrc/phong.hip with it bit for bit; tests/test_phong_cpu.py pins it on the oracle's
frame of T-Rex: against ``oracle.guro`` in the directional, diffuse-only case, by counts, and against itself in float64.

A light is a dict of ``position`` (camera frame) or ``direction`` (the way the light travels: flipped and normalised
as ``GuroIllumination`` does), ``diffuse`` and ``specular``: what ``AdvancedPixelBufferFiller.phong_pass`` takes.

``dtype=np.float64`` evaluates the same statements in double precision from the same float32 barycentrics."""
import numpy as np

import tex_ref

MAX_LIGHTS = 4
MAX_SHININESS_LOG2 = 12


def lights5(lights):
    """(float32 [n, 5]: x, y, z, kd, ks; the mask whose bit j says that light j is a direction): the arguments of
    crender_phong_shade."""
    from oracle import oracle as O
    rows, mask = [], 0
    for j, l in enumerate(lights):
        if "direction" in l:
            vec = O.guro_light(l["direction"])
            mask |= 1 << j
        else:
            vec = np.asarray(l["position"], np.float32)
        rows.append([vec[0], vec[1], vec[2], np.float32(l["diffuse"]), np.float32(l["specular"])])
    return np.array(rows, np.float32).reshape(len(rows), 5), mask


def surface_point(winner, tri, P, y0=0, y1=None):
    """(ys, xs, t, b, z): the covered pixels of the rows, their float32 barycentrics [3][N] and the unprojected z of
    their winners' corners [N, 3]."""
    tri = np.ascontiguousarray(tri, np.float32)
    H, W = winner.shape
    ys, xs, t = tex_ref.covered(winner, tri.shape[0], y0, y1)
    proj = tex_ref.project(tri, P, W, H)
    with np.errstate(all="ignore"):
        b = tex_ref.barycentrics(proj[t], xs, ys)
    return ys, xs, t, b, tri[:, :, 2][t]


def length(a):
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def g(u, n):
    """raster_math.h's guro_factor with `u` as the light; u and n are triples of arrays (or scalars)."""
    d = n[0].dtype.type
    s = ((d(0) + n[0] * u[0]) + n[1] * u[1]) + n[2] * u[2]
    f = s / (length(n) + d(np.float32(1e-6)))
    f = np.where(f < 0, d(0), f)          # (keeps a NaN and a -0)
    return np.where(f > 1, d(1), f)


def light_terms(Pt, Vu, n, vec, directional, shininess_log2):
    """(d, sp) of one light over all pixels, after the `lit` selects."""
    d_ = n[0].dtype.type
    if directional:
        Lu = [np.full_like(n[0], d_(v)) for v in vec]
    else:
        Lv = [d_(vec[c]) - Pt[c] for c in range(3)]
        ll = length(Lv)
        Lu = [Lv[c] / ll for c in range(3)]
    d = g(Lu, n)
    Hv = [Lu[c] + Vu[c] for c in range(3)]
    hl = length(Hv)
    Hu = [Hv[c] / hl for c in range(3)]
    sp = g(Hu, n)
    for _ in range(shininess_log2):
        sp = sp * sp
    lit = d > 0
    d = np.where(lit, d, d_(0))
    sp = np.where(lit & (sp > 0), sp, d_(0))
    return d, sp


def phong_pass(color, winner, tri, P, normals, lights, ambient=0.1, shininess=32, specular_color=(255, 255, 255),
               clamp=255.0, y0=0, y1=None, counts=None, dtype=np.float32):
    """A copy of `color` after crender_phong_shade over rows y0 .. y1 (in `dtype`).  `counts`, a dict, receives the
    number of covered pixels and, per light, of lit, unlit, ``sp > 0`` and ``sp > 0.5`` ones, and the number of pixels
    with a channel at the clamp."""
    k = int(shininess).bit_length() - 1
    assert 1 <= len(lights) <= MAX_LIGHTS and 0 <= k <= MAX_SHININESS_LOG2 and 1 << k == shininess
    d_ = dtype
    L5, mask = lights5(lights)
    out = np.array(color, np.float32, copy=True).astype(d_)
    tri = np.ascontiguousarray(tri, np.float32)
    y1 = out.shape[0] if y1 is None else y1
    ys, xs, t, b, z = surface_point(winner, tri, P, y0, y1)
    with np.errstate(all="ignore"):
        b = [v.astype(d_) for v in b]
        z = z.astype(d_)
        c = tri[t].astype(d_)
        q = [b[k_] / z[:, k_] for k_ in range(3)]
        s = (q[0] + q[1]) + q[2]
        Pt = [((c[:, 0, a] * q[0] + c[:, 1, a] * q[1]) + c[:, 2, a] * q[2]) / s for a in range(3)]
        V = [-Pt[a] for a in range(3)]
        vl = length(V)
        Vu = [V[a] / vl for a in range(3)]
        n = [np.asarray(normals, np.float32)[ys, xs, a].astype(d_) for a in range(3)]
        F = np.full(len(t), d_(np.float32(ambient)))
        Ws = np.zeros(len(t), d_)
        per_light = []
        for j in range(len(lights)):
            d, sp = light_terms(Pt, Vu, n, L5[j, :3], bool(mask >> j & 1), k)
            F = F + d_(L5[j, 3]) * d
            Ws = Ws + d_(L5[j, 4]) * sp
            per_light.append(dict(lit=int((d > 0).sum()), unlit=int((~(d > 0)).sum()), sp_pos=int((sp > 0).sum()),
                                  sp_half=int((sp > 0.5).sum())))
        S = np.asarray(specular_color, np.float32).astype(d_)
        cl = d_(np.float32(clamp))
        o = out[ys, xs] * F[:, None] + Ws[:, None] * S[None, :]
        o = np.where(o > cl, cl, o)
        out[ys, xs] = o
    if counts is not None:
        counts.update(covered=len(t), lights=per_light, clamped=int((o == cl).any(1).sum()) if len(t) else 0)
    return out
