"""Host model of the anisotropic texture pass: the statements of include/crender_aniso.h in vectorised numpy,
one float32 operation per step, on top of tests/mip_ref.py (chain, level rule, trilinear colour) and
tests/tex_ref.py (projection, barycentrics, uv).  The GPU tests compare csrc/texaniso.hip with it bit for bit;
tests/test_aniso_cpu.py pins it by hand and on the four consequences the header states."""
import numpy as np

import mip_ref
import tex_ref

MAX_ANISO = 16


def offsets(N):
    """o_i = (2i + 1 - N) / (2N) for i < N: N points centred on 0, one N-th of the axis apart."""
    i = np.arange(N, dtype=np.int32)
    return (2 * i + 1 - N).astype(np.float32) / np.float32(2 * N)


def footprint(pmax, pmin, A):
    """(rho float32, N int32) of the Footprint and sample count statement."""
    d = np.float32
    pmax, pmin = np.asarray(pmax, d), np.asarray(pmin, d)
    fa = d(A)
    with np.errstate(all="ignore"):
        minified = pmax > d(1)
        lo = pmax / fa
        rho = np.where(pmin >= lo, pmin, lo)
        rho = np.where(rho >= d(1), rho, d(1))
        q = pmax / rho
        many = minified & (q > d(1))
        nf = np.ceil(q)
        below = many & (nf < fa)
    N = np.ones(pmax.shape, np.int32)
    N[many] = A
    N[below] = nf[below].astype(np.int32)
    return np.where(minified, rho, pmax).astype(d), N


def axes(u, v, ux, vx, uy, vy, th, tw):
    """(pmax, pmin, du, dv): the lengths of the major and the minor axis in texels, and the major axis's pair
    of uv differences."""
    d = np.float32
    with np.errstate(all="ignore"):
        dux, dvx, duy, dvy = ux - u, vx - v, uy - u, vy - v
        dudx, dvdx, dudy, dvdy = dux * d(tw), dvx * d(th), duy * d(tw), dvy * d(th)
        rx = dudx * dudx + dvdx * dvdx
        ry = dudy * dudy + dvdy * dvdy
        x_major = rx >= ry                         # a NaN rx makes y the major axis
        pmax = np.sqrt(np.where(x_major, rx, ry))
        pmin = np.sqrt(np.where(x_major, ry, rx))
    return pmax, pmin, np.where(x_major, dux, duy), np.where(x_major, dvx, dvy)


def pixel_footprints(winner, tri, P, uv, th, tw, perspective=False, anisotropy=1, y0=0, y1=None):
    """(ys, xs, u, v, du, dv, N, l0, f) of the covered pixels of the rows."""
    if not (isinstance(anisotropy, int) and 1 <= anisotropy <= MAX_ANISO):
        raise ValueError("anisotropy is an int from 1 to 16")
    tri = np.ascontiguousarray(tri, np.float32)
    H, W = winner.shape
    ys, xs, t = tex_ref.covered(winner, tri.shape[0], y0, y1)
    proj = tex_ref.project(tri, P, W, H)[t]
    uv_t, z_t = np.asarray(uv, np.float32)[t], tri[:, :, 2][t]
    L = len(mip_ref.layout(th, tw)[0])
    with np.errstate(all="ignore"):
        u, v = tex_ref.uv_at(uv_t, z_t, *tex_ref.barycentrics(proj, xs, ys), perspective)
        ux, vx = tex_ref.uv_at(uv_t, z_t, *tex_ref.barycentrics(proj, xs + 1, ys), perspective)
        uy, vy = tex_ref.uv_at(uv_t, z_t, *tex_ref.barycentrics(proj, xs, ys + 1), perspective)
    pmax, pmin, du, dv = axes(u, v, ux, vx, uy, vy, th, tw)
    rho, N = footprint(pmax, pmin, anisotropy)
    l0, f = mip_ref.level_and_weight(rho, L)
    return ys, xs, u, v, du, dv, N, l0, f


def anisotropic(u, v, du, dv, N, l0, f, chain):
    """Colour of each pixel: the trilinear colour where N == 1, else the mean of N trilinear samples along
    the major axis, summed in order."""
    out = np.zeros((len(u), 3), np.float32)
    one = N == 1
    out[one] = mip_ref.trilinear(u[one], v[one], l0[one], f[one], chain)       # no offsets: du * 0 may be NaN
    with np.errstate(all="ignore"):
        for n in np.unique(N[~one]):
            at = N == n
            s = None
            for o in offsets(int(n)):
                c = mip_ref.trilinear(u[at] + du[at] * o, v[at] + dv[at] * o, l0[at], f[at], chain)
                s = c if s is None else s + c
            out[at] = s / np.float32(n)
    return out


def texture_pass(color, winner, tri, P, uv, tex, perspective=False, anisotropy=1, normals=None, light_direction=None,
                 y0=0, y1=None, chain=None):
    """A copy of `color` after crender_aniso_shade over rows y0 .. y1 (mip_ref.texture_pass's arguments)."""
    out = np.array(color, np.float32, copy=True)
    y1 = out.shape[0] if y1 is None else y1
    chain = mip_ref.build_chain(tex) if chain is None else chain
    th, tw = chain[0].shape[:2]
    ys, xs, u, v, du, dv, N, l0, f = pixel_footprints(winner, tri, P, uv, th, tw, perspective, anisotropy, y0, y1)
    out[ys, xs] = anisotropic(u, v, du, dv, N, l0, f, chain)
    if light_direction is not None:
        from oracle import oracle as O
        rows = np.ascontiguousarray(out[y0:y1])
        O.guro(rows, np.ascontiguousarray(normals[y0:y1]), light_direction)
        out[y0:y1] = rows
    return out


def floor_scene():
    """(tri, col, nrm, uv) of a floor receding from z = 0.6 to z = 12 under the camera: two triangles whose
    footprints run from magnified and isotropic (near) to more than sixteen to one (far)."""
    corners = np.float32([[-3, -0.25, 0.6], [3, -0.25, 0.6], [3, -0.25, 12], [-3, -0.25, 12]])
    corner_uv = np.float32([[0, 0], [1, 0], [1, 1], [0, 1]])
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    tri = np.ascontiguousarray(corners[faces])
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1.0
    return tri, np.full_like(tri, 255.0), nrm, np.ascontiguousarray(corner_uv[faces])
