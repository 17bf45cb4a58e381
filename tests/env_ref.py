"""Host model of the environment pass: the statements of include/crender_env.h, "Environment mapping", in vectorised
numpy, one float32 operation per step, over (the winner plane, its unprojected triangles and projection matrix, the normal
plane, the cube map's levels).  Built on ``tex_ref`` (the Bilinear statement, on one face) and ``phong_ref.surface_point``
(the covered pixels and their barycentrics).  The GPU tests compare k_env_shade (csrc/envmap.hip) with it bit for bit;
tests/test_env_cpu.py pins it on the oracle's frames by counts, by identities and against itself in float64.

A cube is uint8 [6, S, S, 3]; `levels` is a list of cubes (``chain_levels``) and `level` a position in it, as
``AdvancedPixelBufferFiller.environment_pass`` takes it.

``dtype=np.float64`` evaluates the same statements in double precision from the same float32 barycentrics and the same
float32 constants."""
import numpy as np

import mip_ref
import phong_ref
import tex_ref

REFLECT, BACKGROUND = 1, 2
MAX_SIDE = 8192


def chain_levels(faces):
    """[cube of side S, S / 2, ..., 1]: the texture chain (tests/mip_ref.py) of the faces stacked by rows, of which the
    levels 0 .. log2 S are six box-averaged faces each."""
    faces = np.ascontiguousarray(np.asarray(faces)[..., :3], np.uint8)
    S = faces.shape[1]
    assert faces.shape == (6, S, S, 3) and S & (S - 1) == 0
    chain = mip_ref.build_chain(faces.reshape(6 * S, S, 3))
    return [chain[j].reshape(6, S >> j, S >> j, 3) for j in range(S.bit_length())]


def pick_levels(levels, level):
    """(faces0, faces1 or None, f float32): the two levels around `level` and the weight of the upper one."""
    l0 = int(np.floor(level))
    assert 0 <= level <= len(levels) - 1
    f = np.float32(level - l0)
    if f >= 1:
        l0, f = l0 + 1, np.float32(0)
    if l0 == len(levels) - 1:
        f = np.float32(0)
    return levels[l0], (levels[l0 + 1] if f != 0 else None), f


def face_of(d):
    """(face, sc, tc, ma) of the directions d, a triple of arrays: the Face statement."""
    a = [np.abs(v) for v in d]
    X = (a[0] >= a[1]) & (a[0] >= a[2])
    Y = ~X & (a[1] >= a[2])
    ma = np.where(X, a[0], np.where(Y, a[1], a[2]))
    dm = np.where(X, d[0], np.where(Y, d[1], d[2]))
    neg = dm < 0
    sc = np.where(X, np.where(neg, d[2], -d[2]), np.where(Y, d[0], np.where(neg, -d[0], d[0])))
    tc = np.where(X, d[1], np.where(Y, np.where(neg, d[2], -d[2]), d[1]))
    return np.where(X, 0, np.where(Y, 2, 4)) + neg, sc, tc, ma


def sample(faces, d):
    """(e [N, 3], usable [N], face [N]) of one level at the directions d."""
    t = d[0].dtype.type
    face, sc, tc, ma = face_of(d)
    usable = (ma > 0) & (ma < np.inf)
    tu = (sc / ma + t(1)) * t(0.5)
    tv = (t(1) - tc / ma) * t(0.5)
    e = np.zeros((len(ma), 3), t)
    for k in range(6):
        at = usable & (face == k)
        if at.any():
            e[at] = tex_ref.bilinear(tu[at], tv[at], faces[k])
    return e, usable, face


def lookup(faces0, faces1, f, M, r):
    """The sample at M r: orientation, one or two levels."""
    t = r[0].dtype.type
    M = np.asarray(M, np.float32).astype(t)
    d = [(M[i, 0] * r[0] + M[i, 1] * r[1]) + M[i, 2] * r[2] for i in range(3)]
    e, usable, face = sample(faces0, d)
    if faces1 is not None:
        up = sample(faces1, d)[0]
        f = t(np.float32(f))
        e = e * (t(1) - f) + up * f
    return e, usable, face


def env_pass(color, winner, tri, P, normals, levels, level=0.0, orientation=None, reflectivity=1.0, f0=0.04,
             tint=(1.0, 1.0, 1.0), background=None, reflect=True, y0=0, y1=None, counts=None, dtype=np.float32):
    """A copy of `color` after crender_env_shade over rows y0 .. y1 (in `dtype`).  `levels` is a cube or a list of
    cubes; `background` None or the gain; `reflect` False drops CRENDER_ENV_REFLECT.  `counts`, a dict, receives the
    number of covered and of written covered pixels, the written ones per face, the background pixels, the written ones
    of them per face, and ``face``, an int plane: the face every written pixel read, -1 elsewhere."""
    t_ = dtype
    if isinstance(levels, np.ndarray):
        levels = [levels]
    faces0, faces1, f = pick_levels(levels, level)
    M = np.eye(3, dtype=np.float32) if orientation is None else np.asarray(orientation, np.float32)
    out = np.array(color, np.float32, copy=True).astype(t_)
    tri = np.ascontiguousarray(tri, np.float32)
    H, W = winner.shape
    y1 = H if y1 is None else y1
    face_map = np.full((H, W), -1, np.int64)
    got = dict(covered=0, written=0, faces=[0] * 6, background=0, background_faces=[0] * 6)
    ys, xs, t, b, z = phong_ref.surface_point(winner, tri, P, y0, y1)
    got["covered"] = len(t)
    if reflect and np.float32(reflectivity) != 0 and len(t):
        with np.errstate(all="ignore"):
            b = [v.astype(t_) for v in b]
            z = z.astype(t_)
            c = tri[t].astype(t_)
            q = [b[k] / z[:, k] for k in range(3)]
            s = (q[0] + q[1]) + q[2]
            p = [((c[:, 0, a] * q[0] + c[:, 1, a] * q[1]) + c[:, 2, a] * q[2]) / s for a in range(3)]
            n = [np.asarray(normals, np.float32)[ys, xs, a].astype(t_) for a in range(3)]
            nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            ni = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]
            k = (t_(2) * ni) / nn
            r = [p[a] - k * n[a] for a in range(3)]
            e, usable, face = lookup(faces0, faces1, f, M, r)
            pp = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
            cs = np.abs(ni) / (np.sqrt(nn) * np.sqrt(pp))
            m = t_(1) - cs
            m = np.where(m < 0, t_(0), m)
            m = np.where(m > 1, t_(1), m)
            ok = usable & (m == m)
            m2 = m * m
            m5 = (m2 * m2) * m
            omf0 = t_(np.float32(1.0 - float(np.float32(f0))))
            w = t_(np.float32(reflectivity)) * (t_(np.float32(f0)) + omf0 * m5)
            T3 = np.asarray(tint, np.float32).astype(t_)
            o = out[ys, xs] * (t_(1) - w)[:, None] + (e * T3[None, :]) * w[:, None]
            out[ys[ok], xs[ok]] = o[ok]
        face_map[ys[ok], xs[ok]] = face[ok]
        got["written"] = int(ok.sum())
        got["faces"] = [int((face[ok] == j).sum()) for j in range(6)]
    if background is not None:
        rows = winner[y0:y1]
        by, bx = np.nonzero(~((rows >= 0) & (rows < tri.shape[0])))
        by = by + y0
        P = np.asarray(P, np.float32).reshape(4, 4)
        xs_, ys_ = np.float32(W / 2.0), np.float32(H / 2.0)
        kx = np.float32(1.0 / (float(xs_) * float(P[0, 0])))
        ky = np.float32(1.0 / (float(ys_) * float(P[1, 1])))
        with np.errstate(all="ignore"):
            r = [(bx.astype(np.float32).astype(t_) - t_(xs_)) * t_(kx), (by.astype(np.float32).astype(t_) - t_(ys_)) * t_(ky),
                 np.ones(len(bx), t_)]
            e, usable, face = lookup(faces0, faces1, f, M, r)
            o = e * t_(np.float32(background))
        out[by[usable], bx[usable]] = o[usable]
        face_map[by[usable], bx[usable]] = face[usable]
        got["background"] = len(bx)
        got["background_faces"] = [int((face[usable] == j).sum()) for j in range(6)]
    if counts is not None:
        counts.update(got, face=face_map)
    return out
