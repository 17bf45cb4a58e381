"""Host model of the deferred shadow pass: the statements of include/crender_shadow.h in vectorised numpy, one
float32 operation per step, over (the camera's winner plane, its unprojected triangles and projection matrix, the
light-frame triangles, the light's projection matrix, its z plane and, optionally, its winner plane).  The GPU tests
compare csrc/shadow.hip with it bit for bit; tests/test_shadow_cpu.py pins it by hand on a floor under an occluder
and on the oracle's frames of T-Rex."""
import numpy as np

import tex_ref

PCF = (1, 3, 5)


def light_point(winner, tri, P, ltri, y0=0, y1=None):
    """(ys, xs, t, X, Y, Z): the covered pixels of the rows and the light-frame coordinates of the surface point
    each one shows — always the perspective-correct blend of the winner's three light-frame corners."""
    tri, ltri = np.ascontiguousarray(tri, np.float32), np.ascontiguousarray(ltri, np.float32)
    H, W = winner.shape
    ys, xs, t = tex_ref.covered(winner, tri.shape[0], y0, y1)
    proj = tex_ref.project(tri, P, W, H)
    with np.errstate(all="ignore"):
        b1, b2, b3 = tex_ref.barycentrics(proj[t], xs, ys)
        z = tri[:, :, 2][t]
        q1, q2, q3 = b1 / z[:, 0], b2 / z[:, 1], b3 / z[:, 2]
        s = (q1 + q2) + q3
        c = ltri[t]
        X, Y, Z = (((c[:, 0, k] * q1 + c[:, 1, k] * q2) + c[:, 2, k] * q3) / s for k in range(3))
    return ys, xs, t, X, Y, Z


def lit_taps(t, X, Y, Z, PL, lz, lwinner, bias, pcf):
    """n, the number of lit taps of each pixel (int, 0 .. pcf * pcf)."""
    from oracle import oracle as O
    assert pcf in PCF
    d = np.float32
    Hl, Wl = lz.shape
    with np.errstate(all="ignore"):
        pts = np.ascontiguousarray(np.stack([X, Y, Z], 1).reshape(-1, 1, 3).repeat(3, 1), np.float32)
        p = O.project(pts, PL, Wl, Hl)[:, 0] if len(pts) else np.zeros((0, 3), np.float32)
        cx = tex_ref.host_i32(np.floor(p[:, 0] + d(0.5))).astype(np.int64)
        cy = tex_ref.host_i32(np.floor(p[:, 1] + d(0.5))).astype(np.int64)
        depth = p[:, 2] - d(bias)
        behind = ~(Z > 0)
        r = (pcf - 1) // 2
        n = np.zeros(len(t), np.int64)
        for j in range(-r, r + 1):
            for i in range(-r, r + 1):
                col, row = cx + i, cy + j
                inside = (col >= 0) & (col < Wl) & (row >= 0) & (row < Hl)
                cc, rr = np.where(inside, col, 0), np.where(inside, row, 0)
                lit = behind | ~inside | ~(depth > lz[rr, cc])
                if lwinner is not None:
                    lit |= inside & (lwinner[rr, cc] == t)
                n += lit
    return n


def factor(n, pcf, ambient):
    """f of the pixels that are written (n < pcf * pcf)."""
    d = np.float32
    frac = n.astype(np.float32) / d(pcf * pcf)
    om = d(1) - d(ambient)
    return d(ambient) + om * frac


def shadow_pass(color, winner, tri, P, ltri, PL, lz, lwinner=None, bias=1e-3, ambient=0.25, pcf=1, y0=0, y1=None,
                counts=None):
    """A copy of `color` after crender_shadow_shade over rows y0 .. y1.  `counts`, a dict, receives the number of
    covered, fully lit (untouched) and fully shadowed pixels."""
    out = np.array(color, np.float32, copy=True)
    y1 = out.shape[0] if y1 is None else y1
    ys, xs, t, X, Y, Z = light_point(winner, tri, P, ltri, y0, y1)
    n = lit_taps(t, X, Y, Z, PL, np.asarray(lz, np.float32), lwinner, bias, pcf)
    w = n < pcf * pcf
    with np.errstate(all="ignore"):
        out[ys[w], xs[w]] = out[ys[w], xs[w]] * factor(n[w], pcf, ambient)[:, None]
    if counts is not None:
        counts.update(covered=len(t), lit=int((n == pcf * pcf).sum()), shadowed=int((n == 0).sum()))
    return out


def rotation_frame(tri, angles):
    """(R float32 [3, 3], t float32 [3]) of the light frame that sees the model rotated by `angles` (degrees about x,
    then y, then z: the matrix of ``Model.rotate``) around the float32 mean of all its corners."""
    a = np.asarray(angles, np.float64) * (np.pi / 180)
    rot2 = [np.array([[np.cos(v), np.sin(v)], [-np.sin(v), np.cos(v)]]) for v in a]
    rx, ry, rz = np.eye(3), np.eye(3), np.eye(3)
    rx[1:, 1:], ry[::2, ::2], rz[:2, :2] = rot2
    R = (rx @ ry @ rz).astype(np.float32)
    c = np.asarray(tri, np.float32).reshape(-1, 3).mean(0, dtype=np.float32)
    return R, (c - R @ c).astype(np.float32)
