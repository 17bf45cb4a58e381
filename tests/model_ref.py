"""numpy models of the entries of csrc/model_ops.hip, one per C entry: every operation spelled out in float32 (or in
float64 where the kernel says so), in the kernel's order, with no BLAS call and no reduction whose order numpy chooses.
tests/test_model_ops_cpu.py pins them against what they restate (GuroIllumination, ``astype('uint8')``, the host
``Model``); tests/test_model_ops_gpu.py holds the kernels to them, bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64
INT_MIN = -2 ** 31


def assert_equal_bits_or_nan(got, want, what):
    """A NaN wherever the model has one, equal bits everywhere else.  (IEEE 754 leaves the sign and the payload of a
    generated NaN open, and x86 and gfx950 differ there: they are not the contract.)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere(gn != wn)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements are NaN on one side only; first at {i}: "
                             f"got {got[i]!r} want {want[i]!r}")
    view = np.uint32 if got.dtype == np.float32 else np.uint64
    g = np.where(wn, got.dtype.type(0), got).view(view)
    w = np.where(wn, want.dtype.type(0), want).view(view)
    bad = np.argwhere(g != w)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; first at {i}: "
                             f"got {got[i]!r} want {want[i]!r}")


# ---- crender_guro_illumination ---------------------------------------------------------------------------------------

def guro(color, normals, light3, y0=0, y1=None):
    """colour[y0:y1] *= clip(n . l / (|n| + 1e-6), 0, 1), in place; rows outside the strip are not touched."""
    with np.errstate(all="ignore"):
        n = normals[y0:y1]
        l0, l1, l2 = (f32(v) for v in light3)
        n0, n1, n2 = n[..., 0], n[..., 1], n[..., 2]
        s = ((f32(0) + n0 * l0) + n1 * l1) + n2 * l2             # the reduction starts from +0
        m = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        c = s / (m + f32(1e-6))
        c = np.where(c < 0, f32(0), c)                           # a NaN and a -0 stay
        c = np.where(c > 1, f32(1), c)
        color[y0:y1] *= c[..., None]
    return color


# ---- crender_present_u8 ----------------------------------------------------------------------------------------------

def present_u8(plane, flip_rows):
    """float32 -> uint8 as x86-64 casts: truncate toward zero to int32, INT_MIN for a NaN and for anything outside
    int32, then the low byte."""
    v = plane[::-1] if flip_rows else plane
    ok = (v >= f32(-2.0 ** 31)) & (v < f32(2.0 ** 31))           # false for a NaN
    with np.errstate(invalid="ignore"):
        iv = np.where(ok, np.trunc(np.where(ok, v, f32(0))).astype(np.int64), INT_MIN)
    return (iv & 0xFF).astype(np.uint8)


# ---- crender_model_shift, crender_model_scale, crender_model_scale3 --------------------------------------------------

def shift(v, s3, in_double):
    """vertices + shift: a float32 sum of the shift rounded to float32, or the float64 sum rounded once."""
    s3 = np.asarray(s3, f64)
    with np.errstate(all="ignore"):
        if in_double:
            return (v.astype(f64) + s3).astype(f32)
        return v + s3.astype(f32)


def scale(v, mean3, c3, in_double, keep):
    """x -= m; x *= c; x += m (keep) or x *= c: the multiply float32, or the float64 product rounded once."""
    c3 = np.broadcast_to(np.asarray(c3, f64), (3,))
    with np.errstate(all="ignore"):
        x = v - mean3 if keep else v.copy()
        x = (x.astype(f64) * c3).astype(f32) if in_double else x * c3.astype(f32)
        return x + mean3 if keep else x


# ---- crender_model_stats ---------------------------------------------------------------------------------------------

def mean_vertex(v):
    """The rows added one after another into a float32 accumulator that starts from +0, as numpy's add.reduce does
    (a column of -0 sums to +0; a cumulative sum is sequential by definition), divided by the count in float64."""
    with np.errstate(all="ignore"):
        acc = np.cumsum(np.concatenate([np.zeros((1, 3), f32), v]), axis=0, dtype=f32)[-1]
        return (acc.astype(f64) / f64(len(v))).astype(f32)


def max_span(v, mean3):
    """max over the vertices of sqrt((dx*dx + dy*dy) + dz*dz) in float32; a NaN anywhere makes it NaN."""
    with np.errstate(all="ignore"):
        d = v - mean3
        r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return f32(np.nan) if np.isnan(r).any() else f32(r.max())


# ---- crender_model_rotate --------------------------------------------------------------------------------------------

def rotate(v, R9):
    """Every coordinate the float64 sum (x*r0 + y*r1) + z*r2 with a row of R9, rounded once to float32."""
    R = np.asarray(R9, f64).reshape(3, 3)
    x, y, z = (v[:, k].astype(f64) for k in range(3))
    with np.errstate(all="ignore"):
        return np.stack([((x * R[j, 0] + y * R[j, 1]) + z * R[j, 2]) for j in range(3)], axis=1).astype(f32)


# ---- crender_model_gather, crender_model_texture_colors --------------------------------------------------------------

def gather(attr, index):
    return attr[index]


def _host_f32_to_i32(t):
    ok = (t >= f32(-2.0 ** 31)) & (t < f32(2.0 ** 31))
    with np.errstate(invalid="ignore"):
        return np.where(ok, np.trunc(np.where(ok, t, f32(0))).astype(np.int64), INT_MIN)


def texture_colors(uv, texture):
    """Nearest texel with the v axis flipped: row = clip(int32((1 - v) * h), 0, h - 1), column = clip(int32(u * w),
    0, w - 1) in float32, the cast INT_MIN for a NaN and outside int32."""
    th, tw = texture.shape[:2]
    with np.errstate(all="ignore"):
        row = np.clip(_host_f32_to_i32((f32(1) - uv[:, 1]) * f32(th)), 0, th - 1)
        colm = np.clip(_host_f32_to_i32(uv[:, 0] * f32(tw)), 0, tw - 1)
    return texture[row, colm, :3].astype(f32)


# ---- crender_model_vertex_normals ------------------------------------------------------------------------------------

def vertex_face_csr(faces, V):
    """DeviceModel._vertex_face_csr's construction: per vertex, the faces of its (face, corner) occurrences in
    ascending order -> (offsets int32 [V + 1], occurrences int32 [3 T])."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    occ = (order // 3).astype(np.int32)
    offs = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=V), out=offs[1:])
    return offs.astype(np.int32), occ


def _dot3_rows(a, b):
    """float32 products added in a double accumulator, rounded once, per row."""
    p = (a * b).astype(f32)
    return ((p[:, 0].astype(f64) + p[:, 1].astype(f64)) + p[:, 2].astype(f64)).astype(f32)


def _unit_rows(n):
    ln = np.sqrt(_dot3_rows(n, n))
    return np.where(ln[:, None] == 0, n, n / ln[:, None]).astype(f32)


def face_normals(vertices, faces):
    """-cross(v1 - v0, v1 - v2) in float32, each product rounded and then the difference, divided by its norm
    unless that is 0 (a NaN norm divides)."""
    with np.errstate(all="ignore"):
        tri = vertices[faces]
        a = tri[:, 1] - tri[:, 0]
        b = tri[:, 1] - tri[:, 2]
        n = np.stack([-(a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]), -(a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]),
                      -(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])], axis=1).astype(f32)
        return _unit_rows(n)


def plain_f32_vertex_normals(vertices, faces, full=False):
    """model.py:175-208 with every operation spelled out (no BLAS call): what the device kernels
    compute, on the host.  A dot of two float32 3-vectors = float32 products summed in float64 and
    rounded once (what numpy's OpenBLAS sdot does, tests/test_host_cpu.py).
    ``full``: -> (normals, face normals, taken), the last one byte per (face, corner) occurrence in
    ``vertex_face_csr``'s order."""
    def dot3(a, b):
        return f32(np.float64(f32(a[0] * b[0])) + np.float64(f32(a[1] * b[1])) + np.float64(f32(a[2] * b[2])))
    fn = face_normals(vertices, faces) if len(faces) else np.zeros((0, 3), f32)
    out = np.zeros((len(vertices), 3), f32)
    buckets = [[] for _ in range(len(vertices))]
    taken = [[] for _ in range(len(vertices))]
    with np.errstate(all="ignore"):
        for t in range(len(faces)):
            for v in faces[t]:
                bk = buckets[v]
                nn = fn[t]
                fresh = not any(dot3(e, nn) >= 1 for e in bk)
                taken[v].append(fresh)
                if fresh:
                    bk.append(nn)
        for v, bk in enumerate(buckets):
            if bk:
                acc = np.zeros(3, f32)
                for e in bk:
                    acc = (acc + e).astype(f32)
                r = (acc.astype(np.float64) / len(bk)).astype(f32)
                l = np.sqrt(dot3(r, r))
                out[v] = r if l == 0 else (r / l).astype(f32)
    if full:
        return out, fn, np.array([b for per in taken for b in per], np.uint8)
    return out


def vertex_normals_one_face_each(vertices, faces):
    """The same for a mesh in which every vertex is named by exactly one face, once, vectorised: the vertex's
    normal is its face's, added to a +0 accumulator, divided by 1 and normalised again.
    -> (normals, face normals)."""
    V = len(vertices)
    flat = np.asarray(faces).reshape(-1)
    assert len(flat) == V and np.array_equal(np.sort(flat), np.arange(V))
    fn = face_normals(vertices, faces)
    with np.errstate(all="ignore"):
        r = (f32(0) + np.repeat(fn, 3, axis=0)).astype(f32)            # (-0 + +0 = +0)
        r = (r.astype(f64) / f64(1)).astype(f32)
        out = np.empty((V, 3), f32)
        out[flat] = _unit_rows(r)
    return out, fn


# ---- crender_tile_order_keys -----------------------------------------------------------------------------------------

def project_rows(v, P, w, h):
    """The oracle's project_vertex on the rows of `v` [n][3]: in place column by column, so column j is formed from
    the already overwritten columns < j; every operation float32, left to right."""
    P = np.asarray(P, f32).reshape(4, 4)
    xs, ys = f32(f64(w) / 2.0), f32(f64(h) / 2.0)
    with np.errstate(all="ignore"):
        c = [v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()]
        z = c[2].copy()
        for j in range(3):
            c[j] = ((c[0] * P[0, j] + c[1] * P[1, j]) + c[2] * P[2, j]) + P[3, j]
        c = [c[0] / z, c[1] / z, c[2] / z]
        c[0] = (c[0] + f32(1)) * xs
        c[1] = (c[1] + f32(1)) * ys
    return np.stack(c, axis=1).astype(f32)


def morton15(x, y):
    """15 bits of x in the even bits, 15 bits of y in the odd ones."""
    x, y = np.asarray(x, np.uint32), np.asarray(y, np.uint32)
    m = np.zeros(x.shape, np.uint32)
    for k in range(15):
        m |= ((x >> np.uint32(k)) & np.uint32(1)) << np.uint32(2 * k)
        m |= ((y >> np.uint32(k)) & np.uint32(1)) << np.uint32(2 * k + 1)
    return m


def tile_order_cells(tri, P, w, h):
    """The pixel (x, y) a triangle's projected centroid is clamped to: the centroid (a + b + c) * float32(1/3) per
    coordinate, projected, truncated and clamped to the frame (in float before the cast: the device's cast
    saturates), both 0 if either is NaN."""
    tri = np.asarray(tri, f32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) * f32(1.0 / 3.0)
        p = project_rows(cen, P, w, h)
        nan = np.isnan(p[:, 0]) | np.isnan(p[:, 1])
        x = np.clip(np.trunc(np.where(nan, f32(0), p[:, 0])), 0, w - 1).astype(np.int64)
        y = np.clip(np.trunc(np.where(nan, f32(0), p[:, 1])), 0, h - 1).astype(np.int64)
    return x, y


def tile_order_keys(tri, P, w, h):
    """Morton code of the 4-pixel cell of the projected centroid."""
    x, y = tile_order_cells(tri, P, w, h)
    return morton15(x >> 2, y >> 2)


# ---- the cases the CPU and the GPU file share ------------------------------------------------------------------------

SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1e-20, -1e-20, 1e10, -1e10,
                     1e19, -1e19, 3e38, -3e38, 1.0, -1.0, 0.5], f32)
LIGHTS = ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.3, -0.2, 1.0), (1e-30, -2e-30, 1.5e-30))
PRESENT_VALUES = np.array([np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 128, -(2.0 ** 31 + 256),
                           2.0 ** 32 + 255, 1e20, 3e9, -3e9, 255.9, -255.9, 256.0, -256.5, 65539.5, -0.0], f32)


def painted_normals(seed, H, W):
    """A normal plane painted with triples of the specials table, a seeded draw with every value in it."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(SPECIALS), H * W * 3)
    idx[:len(SPECIALS)] = np.arange(len(SPECIALS))
    return SPECIALS[idx].reshape(H, W, 3).copy()


def painted_colors(seed, H, W):
    rng = np.random.default_rng(seed)
    color = rng.uniform(-300, 300, (H, W, 3)).astype(f32)
    flat = color.reshape(-1)
    flat[:5] = [-7.5, 0.0, -0.0, np.inf, 255.0]
    return color


def light_vector(light_direction):
    """GuroIllumination.__init__: the light flipped and normalised, float32."""
    flipped = -np.asarray(light_direction, dtype=f32)
    with np.errstate(all="ignore"):                 # (components near 1e-30: the float32 norm is 0, the light infinite)
        return (flipped / np.linalg.norm(flipped)).astype(f32)


def argument_kinds(values, ints=(2, -3, 1)):
    """-> [(name, argument)]: every kind of argument whose promotion against float32 vertices the host Model leaves
    to numpy.  `values`: three floats for the floating kinds (scalars take the first), `ints` for the integer ones."""
    v = [float(x) for x in values]
    k = [int(x) for x in ints]
    return [("Python float", v[0]), ("Python int", k[0]), ("Python bool", True),
            ("list", list(v)), ("tuple", tuple(v)), ("list of ints", list(k)),
            ("np.float16 scalar", np.float16(v[0])), ("np.float32 scalar", f32(v[0])),
            ("np.float64 scalar", f64(v[0])), ("np.int64 scalar", np.int64(k[0])),
            ("0-d float64 array", np.array(v[0], f64)),
            ("float16 array", np.array(v, np.float16)), ("float32 array", np.array(v, f32)),
            ("float64 array", np.array(v, f64)), ("int16 array", np.array(k, np.int16)),
            ("uint8 array", np.array([abs(x) for x in k], np.uint8)), ("bool array", np.array([True, False, True])),
            ("int32 array", np.array(k, np.int32)), ("int64 array", np.array(k, np.int64))]


def special_vertices(rng, V, offset=(10.0, -4.0, 2.0)):
    """Gaussian vertices with rows of specials among them (from V = 85 on)."""
    v = (rng.standard_normal((V, 3)) * [3.0, 1.0, 0.5] + offset).astype(f32)
    if V >= 85:
        v[7] = [np.nan, 1.0, -0.0]
        v[8] = [np.inf, -np.inf, 3e38]
        v[9] = [1e-45, -1e-40, 1e-20]
        v[V - 1] = [-3e38, 0.0, 1e19]
    return v


def boundary_pairs(seed=5, n=40000, cap=60):
    """Pairs of coplanar triangles around a shared corner whose unit normals sit on the boundary of the
    de-duplication test: -> (vertices [5 k][3], faces [2 k][3], kinds [k]) with kind 0 where the dot of the two
    normals is >= 1 as float32 products in a double accumulator but < 1 as a plain float32 sum, and 1 for the
    reverse; the first `cap` pairs of either kind that a draw of `n` candidates holds."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    e1, e2 = q[:, :, 0], q[:, :, 1]
    p = rng.standard_normal((n, 3))

    def corner(a):
        return (p + np.cos(a)[:, None] * e1 + np.sin(a)[:, None] * e2).astype(f32)
    a = rng.uniform(0, 2 * np.pi, (n, 4))
    a[:, 1] = a[:, 0] + rng.uniform(0.3, 2.8, n)          # both triangles counter-clockwise: the same side
    a[:, 3] = a[:, 2] + rng.uniform(0.3, 2.8, n)
    v = np.stack([p.astype(f32), corner(a[:, 0]), corner(a[:, 1]), corner(a[:, 2]), corner(a[:, 3])], axis=1)
    flat = v.reshape(-1, 3)
    base = 5 * np.arange(n)[:, None]
    f1, f2 = base + [0, 1, 2], base + [0, 3, 4]
    n1, n2 = face_normals(flat, f1), face_normals(flat, f2)
    pr = (n1 * n2).astype(f32)
    dd = _dot3_rows(n1, n2)
    plain = ((pr[:, 0] + pr[:, 1]) + pr[:, 2]).astype(f32)
    kind = np.where((dd >= 1) & (plain < 1), 0, np.where((dd < 1) & (plain >= 1), 1, -1))
    keep = np.sort(np.concatenate([np.flatnonzero(kind == 0)[:cap], np.flatnonzero(kind == 1)[:cap]]))
    vertices = v[keep].reshape(-1, 3)
    base = 5 * np.arange(len(keep))[:, None]
    faces = np.stack([base + [0, 1, 2], base + [0, 3, 4]], axis=1).reshape(-1, 3).astype(np.int32)
    return vertices, faces, kind[keep]


def edge_meshes():
    """-> [(name, vertices float32 [V][3], faces int32 [T][3])]: the meshes the vertex normals are held to."""
    rng = np.random.default_rng(41)
    out = []
    v = rng.standard_normal((7, 3)).astype(f32)
    out.append(("first, middle and last vertex unnamed", v, np.array([[1, 2, 4], [4, 5, 2], [5, 1, 2]], np.int32)))
    out.append(("no faces", v[:4].copy(), np.zeros((0, 3), np.int32)))
    out.append(("no vertices", np.zeros((0, 3), f32), np.zeros((0, 3), np.int32)))
    out.append(("a vertex named twice and three times", v[:5].copy(),
                np.array([[0, 0, 1], [2, 2, 2], [0, 1, 2], [3, 4, 3], [1, 3, 4], [4, 1, 4]], np.int32)))
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5], [5, 5, 5], [5, 5, 5], [1, 0, 0], [0, 2, 0]], f32)
    out.append(("collinear and coincident corners", line,
                np.array([[0, 1, 2], [3, 4, 5], [0, 6, 7], [1, 2, 6], [3, 4, 7]], np.int32)))
    ang = np.linspace(0, 2 * np.pi, 201)[:-1] + rng.uniform(0, 1e-3, 200)
    rim = np.stack([np.cos(ang), np.sin(ang), np.zeros(200)], axis=1)
    cone = np.concatenate([[[0.0, 0.0, 1.0]], rim]).astype(f32)
    k = np.arange(200)
    out.append(("a fan of 200 faces with distinct normals", cone,
                np.stack([np.zeros(200, int), 1 + k, 1 + (k + 1) % 200], axis=1).astype(np.int32)))
    ang = np.sort(rng.uniform(0, 2 * np.pi, 65))
    rad = rng.uniform(0.5, 2.0, 65)
    disc = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(65)], 1)])
    k = np.arange(64)
    out.append(("a fan of 64 coplanar faces", disc.astype(f32),
                np.stack([np.zeros(64, int), 1 + k, 2 + k], axis=1).astype(np.int32)))
    bv, bf, _ = boundary_pairs()
    out.append(("boundary pairs", bv, bf))
    w = rng.standard_normal((9, 3)).astype(f32)
    w[3] = [np.nan, 0.5, 0.25]
    w[6] = [1.0, np.inf, -2.0]
    out.append(("a NaN corner and an inf corner", w,
                np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [1, 5, 6], [1, 6, 7], [1, 7, 8], [2, 7, 8]], np.int32)))
    big = (rng.standard_normal((6, 3)) * 1e20).astype(f32)
    big[5] = [0.5, 0.25, -1.0]
    out.append(("corners at 1e20", big, np.array([[0, 1, 2], [2, 3, 4], [0, 4, 5], [1, 3, 5]], np.int32)))
    tiny = (rng.standard_normal((6, 3)) * 1e-12).astype(f32) + f32(0.0)
    out.append(("triangles of side 1e-12", tiny, np.array([[0, 1, 2], [2, 3, 4], [0, 4, 5], [1, 3, 5]], np.int32)))
    return out


def key_triangles(rng, T, res):
    """Triangles for the tile-order keys: a soup whose centroids spread beyond all four sides of the frame, and, from
    T = 257 on, centroids behind the camera, NaN and +-inf corners and corners of 3e38 whose sum overflows."""
    f = 2.4142137
    cz = rng.uniform(0.5, 3.0, (T, 1))
    cxy = rng.uniform(-1.6 / f, 1.6 / f, (T, 2)) * cz
    centre = np.concatenate([cxy, cz], 1)[:, None, :]
    tri = (centre + rng.uniform(-1, 1, (T, 3, 3)) * (8.0 / res) * cz[:, None, :]).astype(f32)
    if T >= 257:
        tri[10:20, :, 2] *= -1                                        # behind the camera
        tri[20, 0, 0], tri[21, 1, 1], tri[22, 2, 2] = np.nan, np.nan, np.nan
        tri[23, 0, 0], tri[24, 1, 1], tri[25, 2, 2] = np.inf, -np.inf, np.inf
        tri[26, 0, 0], tri[26, 1, 0] = np.inf, -np.inf
        tri[27, :, 0], tri[28, :, 1], tri[29, :, 2] = 3e38, -3e38, 3e38
        tri[30, :, :2] = 0.0                                          # the frame's centre
        tri[31] = 0.0                                                 # z = 0
    return tri
