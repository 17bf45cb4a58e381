"""Hand-built edge scenes for the deferred passes (texture, mip, aniso, shadow, Phong, occlusion), shared by tests/test_pass_edges_cpu.py
and tests/test_pass_edges_gpu.py.  Pure numpy on top of the host models (tests/tex_ref.py and its companions): a small
frame whose winner plane is PAINTED, block by block, not rasterized, so that the passes meet operands no rasterizer
hands them — pixels far outside their winner, triangles of no area or of 10^13 px^2, corners at z = 2^-43 or NaN —
and every window decision of the shared-reciprocal shortcut is taken both ways.  (The float32 projection is
tex_ref.project's, the oracle's C restatement: users build the oracle first, as the `oracle` fixture does.)

The decisions, in the kernels' order (csrc/raster_math.h states the window: "When |d| and |n| both lie in
[2^-40, 2^40] neither div_scale changes its operand and div_fmas is a plain fma ... Outside the window (and for
n == 0) the full `/` is used."):
    fast    the three denominators l03, l13, l23 of the barycentrics are inside the window         (per triangle)
    num     the smallest |numerator| is >= 2^-40 and the largest <= 2^40                           (per point)
    z_fast  the three corners' unprojected z are inside the window                                 (per triangle)
    b       the three barycentrics are inside the window                                           (per point)
    s       s, nu and nv of the Perspective statement are inside the window                        (per point)
`classify` restates them in numpy float32 from the host model's own operands; no kernel code is imported.

The Phong and the occlusion pass take no such shortcut; what they add to the scenes (`_lit`, at the end: a z plane,
tap tables, light sets) is drawn after everything else, so that the arrays of the four older passes stay what they were.

Nor do the two wire passes (the overlay and the outline).  `_wired`, after `_lit`, gives the scenes an edge mask — and
the tall frame a z plane — from generators of its own; and three frames at the end are theirs alone: `tie_scene` (the
hidden-line test at equality, the three sides of the clamp, the NaN), `sparse_frames` and `sparse_strip` (lone winners
on the seams of the outline's 32 x 32 tiles, for the rows a wavefront skips)."""
import functools

import numpy as np

import ao_ref
import outline_ref
import phong_ref
import shadow_ref
import tex_ref

H, W = 84, 100                       # 11 x 13 blocks of 8 x 8 pixels, the last row and column of them partial
BLOCK = 8
DIV_LO, DIV_HI = np.float32(2.0 ** -40), np.float32(2.0 ** 40)      # raster_math.h: the window [2^-40, 2^40]
DECISIONS = ("fast", "num", "z_fast", "b", "s")
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31

# A projection whose entries are powers of two: x' = 2 x / z, y' = 2 y / z, z' = 1 - 0.25 / z, so that screen
# coordinates can be hit exactly (crender_project reads the first three columns only).
P = np.float32([[2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 1], [0, 0, -0.25, 0]])
HL, WL = 42, 50                      # the shadow map: the same projection at half the resolution
BIAS = 1e-3
LIGHT = (0.3, -0.2, 1.0)             # what GuroIllumination is constructed with


def in_window(a):
    """raster_math.h's window test: false for NaN, inf and 0."""
    with np.errstate(all="ignore"):
        m = np.abs(a)
        return (m >= DIV_LO) & (m <= DIV_HI)


def unproject(sx, sy, z, w=W, h=H):
    """Model-space corners [.., 3] float32 that project near screen (sx, sy) at depth z under P."""
    sx, sy, z = (np.asarray(v, np.float64) for v in (sx, sy, z))
    x = (sx / (w / 2.0) - 1.0) * z / 2.0
    y = (sy / (h / 2.0) - 1.0) * z / 2.0
    return np.stack(np.broadcast_arrays(x, y, z), -1).astype(np.float32)


def edge_terms(proj, xs, ys):
    """(l03, l13, l23, n1, n2, n3) of math_utils.pyx:8-34 in the arrays' dtype: tex_ref.barycentrics before the division."""
    d = proj.dtype.type
    x0, y0, x1, y1, x2, y2 = proj[:, 0, 0], proj[:, 0, 1], proj[:, 1, 0], proj[:, 1, 1], proj[:, 2, 0], proj[:, 2, 1]
    fx, fy = xs.astype(d), ys.astype(d)
    with np.errstate(all="ignore"):
        l01, l02 = x1 - x2, y1 - y2
        l03 = l01 * (y0 - y2) - l02 * (x0 - x2)
        l11, l12 = x2 - x0, y2 - y0
        l13 = l11 * (y1 - y0) - l12 * (x1 - x0)
        l21, l22 = x0 - x1, y0 - y1
        l23 = l21 * (y2 - y1) - l22 * (x2 - x1)
        n1 = l01 * (fy - y2) - l02 * (fx - x2)
        n2 = l11 * (fy - y0) - l12 * (fx - x0)
        n3 = l21 * (fy - y1) - l22 * (fx - x1)
    return l03, l13, l23, n1, n2, n3


class Scene:
    """tri, uv, ltri [T, 3, ..] float32, classes {name: [triangle ids]}, winner int32 [H, W], colour and normal planes,
    the shadow map (lz, lwinner) and a pos_of permutation.  Built once (`scene()`), only read afterwards."""


def _build():
    rng = np.random.default_rng(20240)
    tris, uvs, ltris, classes = [], [], [], {}
    d = np.float32

    def add(cls, tri, uv=None, ltri=None):
        tri = np.asarray(tri, np.float32).reshape(3, 3)
        uv = rng.uniform(0, 1, (3, 2)) if uv is None else uv
        classes.setdefault(cls, []).append(len(tris))
        tris.append(tri)
        uvs.append(np.asarray(uv, np.float32).reshape(3, 2))
        ltris.append(tri.copy() if ltri is None else np.asarray(ltri, np.float32).reshape(3, 3))
        return len(tris) - 1

    def screen(pts, z):
        pts = np.asarray(pts, np.float64)
        return unproject(pts[:, 0], pts[:, 1], np.broadcast_to(np.asarray(z, np.float64), (3,)))

    # ordinary: large triangles over the frame, corners at different depths; uv from magnified to strongly minified,
    # light frames: the camera's own, a turned one, one beside the map, one behind the light, one beyond int32
    big = [[(-10, -8), (120, 10), (30, 100)], [(110, 90), (-20, 70), (60, -15)], [(5, 5), (95, 20), (50, 80)],
           [(-30, 40), (130, 45), (50, -60)], [(0, 84), (100, 84), (50, -10)], [(20, -5), (105, 50), (-5, 60)],
           [(-15, -15), (115, -10), (110, 95)], [(-12, 95), (-8, -12), (112, 40)]]
    R, t = shadow_ref.rotation_frame(screen(big[0], 1.0), (6, -9, 0))
    for k, pts in enumerate(big):
        tri = screen(pts, rng.uniform(1.0, 1.8, 3) if k < 2 else rng.uniform(0.5, 3.0, 3))
        uv = rng.uniform(0, 1, (3, 2)) * [1, 1, 4, 4, 16, 16, 64, 300][k]
        ltri = [None, (tri @ R.T + t), tri + d([3.0, 0, 0]), tri * d([1, 1, -1]), tri * d([1e12, 1, 1]), None, None,
                (tri @ R.T + t)][k]
        add("ordinary", tri, uv, ltri)
    # small: a hundredth of a pixel across, every denominator still inside the window: barycentrics of 10^3 .. 10^7
    for size in (3e-2, 1e-2, 4e-3):
        c = rng.uniform(20, 70, 2)
        add("small", screen(c + size * rng.uniform(-1, 1, (3, 2)), rng.uniform(0.8, 2.0, 3)))
    # zero: no area at all (0 / 0 and n / 0).  (A denominator under 2^-40 that is NOT zero needs a smaller frame:
    # see mini_scene.)
    p = screen([(30, 30), (60, 50), (45, 40)], 1.0)
    add("zero", np.stack([p[0], p[0], p[1]]))
    add("zero", np.stack([p[0], p[0], p[0]]))
    add("zero", [[0, 0, 1], [0.25, 0.25, 1], [0.5, 0.5, 1]])      # exactly (50, 42), (75, 63), (100, 84): one line
    # huge: corners millions of pixels outside the frame, more than 2^40 px^2
    add("huge", screen([(-3e6, -2e6), (4e6, -1e6), (1e5, 5e6)], [0.7, 1.0, 2.0]))
    add("huge", screen([(50, 40), (6e6, 3e6), (-5e6, 4e6)], 1.0))
    # corners' z below and above the window, x and y scaled along so the corners still project apart
    # (each corner alone, too: a window test forgotten for one operand shows only there)
    for name, zs in (("z_low", [(1e-13, 1.0, 2.0), (2e-13, 1e-13, 4e-13), (1.0, 3e-13, 2.0), (1.0, 2.0, 1e-13), (1.5, 1.0, 1e-38)]),
                     ("z_high", [(4e12, 1.0, 2.0), (4e12, 3e12, 8e12), (1.5, 4e12, 1.0), (1.0, 2.0, 4e12), (1.0, 1.5, 1e38)]),
                     ("z_edge", [(2.0 ** 40,) * 3, (2.0 ** 39, 2.0 ** 40, 2.0 ** 40), (2.0 ** 39,) * 3,
                                 (2.0 ** 40, 2.0 ** 39, 2.0 ** 39), (2.0 ** -40, 2.0 ** -40, 2.0 ** -39),
                                 (2.0 ** 38,) * 3, (2.0 ** 39, 2.0 ** 39, 2.0 ** 38),
                                 (2.0 ** 37, 2.0 ** 38, 2.0 ** 39), (2.0 ** 39, 2.0 ** 38, 2.0 ** 38)])):
        for k, z in enumerate(zs):
            add(name, screen(big[(k + 2) % len(big)], z))
    # corners whose z is no depth at all
    for k, z in enumerate([0.0, -1.0, np.nan, np.inf, -np.inf, -0.0]):
        tri = screen(big[k % len(big)], 1.5)
        tri[k % 3, 2] = z
        add("z_bad", tri)
    # an infinite z at each corner alone.  (crender_project forms x * P00 + y * P10 + z * P20 + P30 first: inf * 0, or
    # inf / inf after it, is a NaN whatever the matrix, so the corner's screen position, the barycentrics and the
    # colour are NaN on every path; tests/test_pass_edges_cpu.py says so.)
    for k, (corner, z) in enumerate([(2, np.inf), (2, -np.inf), (0, np.inf), (1, -np.inf), (1, np.inf), (0, -np.inf)]):
        tri = screen(big[(k + 3) % len(big)], rng.uniform(0.8, 2.5, 3))
        tri[corner, 2] = z
        add("z_inf", tri)
    # z_far: ONE corner at z = 10^38 and the only live uv at that corner, sized so that u = u_c (b_c / z_c) / s is of
    # the size of a texture: the quotient b_c / z_c is a subnormal number, `/` rounds it correctly, and uv is made of
    # nothing else — a window test forgotten for that corner's z shows in the colour
    for k, corner in enumerate((2, 1, 2, 0)):
        zs = np.array(rng.uniform(0.8, 2.0, 3))
        zs[corner] = 1e38
        uv = np.zeros((3, 2))
        uv[corner] = [3e37, 1.2e38] if k < 2 else [-1e38, 2e37]
        add("z_far", screen(big[k + 1], zs), uv)
    # aligned: a corner at the centre of the frame (x = y = 0 projects to exactly W / 2, H / 2) and two edges along
    # its row and its column: the numerators of every pixel of that row and column are exactly zero
    for a, b in ((0.9, 0.8), (-0.9, 0.7), (0.8, -0.9), (-0.7, -0.8)):
        z = float(rng.uniform(0.8, 2.0))
        add("aligned", [[0, 0, z], [a * z, 0, z], [0, b * z, z]])
    # uv columns that are all zero (nu == 0), uv of 10^13 (nu beyond 2^40), NaN and infinite uv (a NaN rho)
    for k, uv in enumerate([np.zeros((3, 2)), rng.uniform(0, 1, (3, 2)) * [0, 1], rng.uniform(0, 1, (3, 2)) * [1, 0]]):
        add("uv_zero", screen(big[k], rng.uniform(0.5, 3.0, 3)), uv)
    for k in range(3):                                        # two corners' uv zero, the third live: nu IS its term
        uv = np.zeros((3, 2))
        uv[k] = rng.uniform(0.3, 1, 2) * [1, 1e30, 40][k]
        add("uv_zero", screen(big[k + 4], rng.uniform(0.5, 3.0, 3)), uv)
    for k, scale in enumerate([1e13, -3e13, 5e12]):
        add("uv_big", screen(big[k + 3], rng.uniform(0.5, 3.0, 3)), rng.uniform(0.2, 1, (3, 2)) * scale)
    for k, odd in enumerate([np.nan, np.inf, -np.inf]):
        uv = rng.uniform(0, 1, (3, 2))
        uv[k, k % 2] = odd
        add("uv_nan", screen(big[k + 5], rng.uniform(0.5, 3.0, 3)), uv)
    # pow2: corners at (0, 0), (64, 0), (0, 64) px and z = 1, v = c y and u the same at every corner: rho is the rounded
    # difference of two v, times th: for th = 64 it lands on c * 64 = 1, 2, 8, 64, .. EXACTLY at a good share of the
    # pixels and an ulp or two to either side at the others (rho == 1, rho just over and just under it, f == 0 on a
    # level above the first)
    corner = screen([(0, 0), (64, 0), (0, 64)], 1.0)
    for k, c in enumerate((1 / 64, 1 / 64, 2 / 64, 2 / 64, 8 / 64, 1.0, 512.0, (1 + 2.0 ** -20) / 64, (1 - 2.0 ** -20) / 64,
                           (1 + 2.0 ** -19) / 64, (1 - 2.0 ** -19) / 64, (1 + 2.0 ** -21) / 64, (1 - 2.0 ** -21) / 64)):
        add("pow2", corner, [[0.5 * (k % 2), 0], [0.5 * (k % 2), 0], [0.5 * (k % 2), 64 * c]])
    # rho: uv steps of a quarter, one and a hundred texture widths per pixel: at and beyond the coarsest level of any chain
    for k, step in enumerate([0.25, 0.5, 1.0, 100.0]):
        add("rho", screen(big[k], 1.0 + k), rng.uniform(0, 1, (3, 2)) * step * 100)
    # aniso: u = a (sx + 100), v = b (sy + 100) over the whole frame: footprints of (k - 1/2) to 1 for a texture of
    # 64 x 97 texels (th x tw), so that crender_aniso_shade takes every N from 1 to 16 at A = 16 (and the clamp at
    # A = 2 and 4)
    for k in range(1, 19):
        a, b = (k - 0.5) * 1.5 / 97, 1.5 / 64
        if k % 2:
            a, b = b * 64 / 97, a * 97 / 64             # (odd k: y is the major axis)
        add("aniso", screen([(-100, -100), (300, -100), (-100, 300)], 1.0), [[0, 0], [400 * a, 0], [0, 400 * b]])

    s = Scene()
    s.tri, s.uv, s.ltri = (np.ascontiguousarray(np.stack(v), np.float32) for v in (tris, uvs, ltris))
    s.classes = classes
    s.T = T = len(tris)
    s.H, s.W = H, W
    s.class_of = np.empty(T, object)
    for name, ids in classes.items():
        s.class_of[ids] = name

    # ---- the winner plane, painted in the kernels' 8 x 8 blocks ----------------------------------------------------
    by, bx = (H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK
    nb = by * bx
    kinds = [("one", t) for ids in classes.values() for t in ids[:2]]                   # a single triangle: uniform
    kinds += [("one", t) for t in classes["aniso"][2:]]
    kinds += [("background", None)] * 6
    names = list(classes)
    while len(kinds) < nb:
        k = len(kinds) % 3
        kinds.append(("all", None) if k == 0 else ("classes", list(rng.choice(names, 3, replace=False))) if k == 1
                     else ("far", None))
    order = rng.permutation(nb)
    winner = np.full((H, W), -1, np.int32)
    single = np.zeros((H, W), bool)                           # blocks of one triangle stay whole: a uniform branch
    weights = np.array([8.0 if s.class_of[t] == "ordinary" else 1.0 for t in range(T)])
    weights /= weights.sum()
    for slot, (kind, arg) in zip(order, kinds):
        r, c = divmod(int(slot), bx)
        blk = winner[r * BLOCK:(r + 1) * BLOCK, c * BLOCK:(c + 1) * BLOCK]
        if kind == "one":
            blk[:] = arg
            single[r * BLOCK:(r + 1) * BLOCK, c * BLOCK:(c + 1) * BLOCK] = True
        elif kind == "all":                                   # every class, lane by lane
            blk[:] = rng.choice(T, blk.shape, p=weights)
        elif kind == "classes":
            blk[:] = rng.choice(np.concatenate([classes[n] for n in arg]), blk.shape)
        elif kind == "far":                                   # winners nowhere near: negative and huge barycentrics
            blk[:] = rng.choice(classes["small"] + classes["aligned"] + classes["ordinary"][:3], blk.shape)
    # every other pixel of the centre row and column to the aligned triangles: numerators that are exactly zero
    line = np.zeros((H, W), bool)
    line[H // 2, ::2] = line[1::2, W // 2] = True
    line &= ~single
    winner[line] = rng.choice(classes["aligned"], int(line.sum()))
    bad = np.int32([-1, -7, T, T + 5, INT_MAX, INT_MIN])
    hit = (rng.uniform(size=winner.shape) < 0.04) & ~single
    winner[hit] = rng.choice(bad, int(hit.sum()))
    at = np.nonzero(~single.reshape(-1))[0][:len(bad)]        # (each of them at least once)
    winner.reshape(-1)[at] = bad
    s.winner = winner
    s.color = rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
    nrm = rng.standard_normal((H, W, 3)).astype(np.float32)
    nrm[..., 2] = -np.abs(nrm[..., 2])
    nrm[rng.uniform(size=(H, W)) < 0.1] = 0                   # (a background's normal)
    s.normals = nrm

    # ---- d_pos_of: the triangles moved, one of them (an ordinary one) sent beyond T: its pixels are background -------
    perm = rng.permutation(T).astype(np.uint32)
    s.moved = np.empty_like(s.tri)
    s.moved[perm] = s.tri
    s.gone = int(classes["ordinary"][2])
    s.pos_of = perm.copy()
    s.pos_of[s.gone] = T + 3
    s.winner_without_gone = np.where(winner == s.gone, -1, winner).astype(np.int32)

    # ---- the shadow map: depths equal to a pixel's own depth minus the bias, one ulp either side, NaN, infinities ---
    ys, xs, t, cx, cy, depth, behind = shadow_points(s, winner)
    lz = rng.uniform(0.3, 1.0, (HL, WL)).astype(np.float32)
    lwinner = rng.integers(-1, T, (HL, WL)).astype(np.int32)
    ok = ~behind & (cx >= 0) & (cx < WL) & (cy >= 0) & (cy < HL) & np.isfinite(depth)
    idx = np.nonzero(ok)[0]
    kind = (xs[idx] + 2 * ys[idx] + (xs[idx] // 2) + (ys[idx] // 2)) % 6
    up = np.nextafter(depth[idx], d(np.inf), dtype=d)
    down = np.nextafter(depth[idx], d(-np.inf), dtype=d)
    value = np.where(kind == 0, depth[idx], np.where(kind == 1, up, np.where(kind == 2, down, d(0))))
    put = kind < 3
    lz[cy[idx][put], cx[idx][put]] = value[put].astype(d)
    own = kind == 4                                           # the light saw this very triangle: lit whatever the depths say
    lz[cy[idx][own], cx[idx][own]] = d(-1.0)
    lwinner[cy[idx][own], cx[idx][own]] = t[idx][own]
    odd = rng.uniform(size=lz.shape) < 0.06
    lz[odd] = rng.choice(d([np.nan, np.inf, -np.inf, 1e6]), int(odd.sum()))
    hit = rng.uniform(size=lwinner.shape) < 0.05
    lwinner[hit] = rng.choice(bad, int(hit.sum()))
    lz[2:14, 2:24] = d(-2.0)                                  # a solid occluder: every tap of a pixel under it is shadowed
    lwinner[2:14, 2:24] = -1
    s.lz, s.lwinner = lz, lwinner
    return s


def shadow_points(s, winner, bias=BIAS):
    """(ys, xs, t, cx, cy, depth, behind) of the covered pixels: the centre texel and the depth the shadow model
    (tests/shadow_ref.py) compares with the map."""
    d = np.float32
    ys, xs, t, X, Y, Z = shadow_ref.light_point(winner, s.tri, P, s.ltri)
    with np.errstate(all="ignore"):
        pts = np.ascontiguousarray(np.stack([X, Y, Z], 1).reshape(-1, 1, 3).repeat(3, 1), np.float32)
        p = tex_ref.project(pts, P, WL, HL)[:, 0] if len(pts) else np.zeros((0, 3), np.float32)
        cx = tex_ref.host_i32(np.floor(p[:, 0] + d(0.5))).astype(np.int64)
        cy = tex_ref.host_i32(np.floor(p[:, 1] + d(0.5))).astype(np.int64)
        depth = p[:, 2] - d(bias)
        behind = ~(Z > 0)
    return ys, xs, t, cx, cy, depth, behind


@functools.lru_cache(maxsize=None)
def scene():
    return _wired(_lit(_build(), 20244), 20246)


def classify(s, winner=None, dtype=np.float32):
    """The operands of every decision, recomputed with the host model's statements: a dict with ys, xs, t of the
    covered pixels and, per decision, a bool [N, 3] that is True where the point — (x, y), (x + 1, y), (x, y + 1) —
    takes the FAST side (the shortcut), False where it takes `/`."""
    winner = s.winner if winner is None else winner
    ys, xs, t = tex_ref.covered(winner, s.T)
    proj = tex_ref.project(s.tri, P, s.W, s.H, dtype)[t].astype(dtype)
    uv_t, z_t = s.uv.astype(dtype)[t], s.tri[:, :, 2].astype(dtype)[t]
    out = {"ys": ys, "xs": xs, "t": t}
    sides = {k: [] for k in DECISIONS}
    with np.errstate(all="ignore"):
        for dx, dy in ((0, 0), (1, 0), (0, 1)):
            l03, l13, l23, n1, n2, n3 = edge_terms(proj, xs + dx, ys + dy)
            sides["fast"].append(in_window(l03) & in_window(l13) & in_window(l23))
            lo = np.fmin(np.fmin(np.abs(n1), np.abs(n2)), np.abs(n3))           # fminf / fmaxf: a NaN is passed over
            hi = np.fmax(np.fmax(np.abs(n1), np.abs(n2)), np.abs(n3))
            sides["num"].append((lo >= DIV_LO) & (hi <= DIV_HI))
            sides["z_fast"].append(in_window(z_t[:, 0]) & in_window(z_t[:, 1]) & in_window(z_t[:, 2]))
            b1, b2, b3 = tex_ref.barycentrics(proj, xs + dx, ys + dy)
            sides["b"].append(in_window(b1) & in_window(b2) & in_window(b3))
            q1, q2, q3 = b1 / z_t[:, 0], b2 / z_t[:, 1], b3 / z_t[:, 2]
            sm = (q1 + q2) + q3
            nu = (uv_t[:, 0, 0] * q1 + uv_t[:, 1, 0] * q2) + uv_t[:, 2, 0] * q3
            nv = (uv_t[:, 0, 1] * q1 + uv_t[:, 1, 1] * q2) + uv_t[:, 2, 1] * q3
            sides["s"].append(in_window(sm) & in_window(nu) & in_window(nv))
    for k in DECISIONS:
        out[k] = np.stack(sides[k], 1)
    return out


# ---- the small frame: denominators under 2^-40 that are not zero -----------------------------------------------------

MINI_H, MINI_W = 20, 28


@functools.lru_cache(maxsize=None)
def mini_scene():
    """crender_project ends in (v + 1) * (W / 2), and v + 1 is a multiple of 2^-24: projected corners lie on a grid
    of W / 2 * 2^-24 by H / 2 * 2^-24 px, the three denominators of a triangle (each twice its area, formed without
    a rounding at this size) are whole multiples of one grid cell, and a cell is under 2^-40 px^2 only when
    W * H < 1024.  On this 28 x 20 frame a cell is 140 * 2^-48 = 2^-40.9 px^2: triangles of three neighbouring grid
    points next to the frame's corner have denominators under the window that are not zero."""
    rng = np.random.default_rng(20242)
    s = Scene()
    s.H, s.W = MINI_H, MINI_W
    q = 2.0 ** -24
    tris = []
    for k0, m0, dk, dm in ((3000, 5000, 1, 1), (70000, 900, -1, 1), (123456, 654321, 1, -1)):
        grid = np.float64([[k0, m0], [k0 + dk, m0], [k0, m0 + dm]]) * q - 1.0          # x' / z, y' / z
        tris.append(np.concatenate([grid / 2.0, np.ones((3, 1))], 1).astype(np.float32))
    for pts in ([(-3, -2), (33, 4), (10, 25)], [(30, 22), (-5, 18), (14, -6)], [(2, 1), (26, 3), (13, 19)]):
        pts = np.float64(pts)
        tris.append(unproject(pts[:, 0], pts[:, 1], rng.uniform(0.5, 3.0, 3), MINI_W, MINI_H))
    s.tri = np.ascontiguousarray(np.stack(tris), np.float32)
    s.T = T = len(tris)
    s.classes = {"tiny": [0, 1, 2], "ordinary": [3, 4, 5]}
    s.uv = rng.uniform(0, 1, (T, 3, 2)).astype(np.float32)
    s.uv[3:] *= np.float32([[[1]], [[8]], [[64]]])
    s.ltri = s.tri.copy()
    s.winner = rng.integers(-1, T + 1, (MINI_H, MINI_W)).astype(np.int32)
    s.winner[:8, :8] = 0                                      # a wavefront of one tiny triangle, the others mixed
    s.color = rng.uniform(0, 255, (MINI_H, MINI_W, 3)).astype(np.float32)
    nrm = rng.standard_normal((MINI_H, MINI_W, 3)).astype(np.float32)
    nrm[..., 2] = -np.abs(nrm[..., 2])
    s.normals = nrm
    s.lz = rng.uniform(0.3, 1.0, (HL, WL)).astype(np.float32)
    s.lwinner = rng.integers(-1, T, (HL, WL)).astype(np.int32)
    return _wired(_lit(s, 20245), 20247)


# ---- the tall frame: more 8-row blocks than a grid is tall ----------------------------------------------------------

TALL_H, TALL_W, TALL_Y0 = 524296, 3, 3        # rows 3 .. H: 65 537 blocks, the last one partial; a grid has 65 535


@functools.lru_cache(maxsize=None)
def tall_scene():
    """A frame of 524 296 x 3 pixels that is background but for its first rows, the rows around 524 280 (the first
    ones of the loop's second trip) and the last, partial block: (tri, uv, ltri, winner, colour, normals)."""
    rng = np.random.default_rng(20241)
    s = Scene()
    tris, uvs = [], []
    for top in (0, TALL_H - 40):
        for k in range(4):
            pts = np.stack([rng.uniform(-6, 9, 3), top + rng.uniform(-10, 50, 3)], 1)
            tris.append(unproject(pts[:, 0], pts[:, 1], rng.uniform(0.5, 3.0, 3), TALL_W, TALL_H))
            uvs.append(rng.uniform(0, 1, (3, 2)) * [1, 4, 16, 64][k])
    s.tri = np.ascontiguousarray(np.stack(tris), np.float32)
    s.uv = np.ascontiguousarray(np.stack(uvs), np.float32)
    s.T = T = len(tris)
    s.H, s.W = TALL_H, TALL_W
    s.ltri = s.tri.copy()
    s.ltri[1::2] += np.float32([0.0, 0.0, 0.25])
    winner = np.full((TALL_H, TALL_W), -1, np.int32)
    winner[:20] = rng.integers(-1, 4, (20, TALL_W))
    winner[TALL_H - 30:] = rng.integers(3, T + 1, (30, TALL_W))           # (T itself names no triangle)
    s.winner = winner
    s.rows = np.r_[0:24, TALL_H - 34:TALL_H]                              # where anything can differ without a light
    s.color = rng.uniform(0, 255, (TALL_H, TALL_W, 3)).astype(np.float32)
    nrm = rng.standard_normal((TALL_H, TALL_W, 3)).astype(np.float32)
    nrm[..., 2] = -np.abs(nrm[..., 2])
    s.normals = nrm
    # the light looks along the camera's axis at a small map: the tall frame's columns fall into its middle
    s.lz = rng.uniform(0.3, 1.0, (HL, WL)).astype(np.float32)
    s.lwinner = rng.integers(-1, T, (HL, WL)).astype(np.int32)
    s.lights = light_sets(s, None)
    return _wired(s, 20248, z=True)


# ---- what the Phong and the occlusion pass need: drawn after everything above, from generators of their own ----------

# tests/test_ao_gpu.py's table of 16 taps within 8 px, and the corners and edge midpoints of the largest halo
TABLE = [(1, 0), (-2, 2), (0, -3), (2, 3), (-4, -1), (4, -3), (-1, 5), (-3, -5), (5, 2), (-6, 2), (3, -6), (2, 6), (-6, -4),
         (7, -2), (-4, 6), (-1, -8)]
HALO_TABLE = [(32, 32), (-32, 32), (32, -32), (-32, -32), (32, 0), (-32, 0), (0, 32), (0, -32)]
POINT = (0.1, -0.1, 1.5)             # inside the depth range of the "ordinary" triangles (0.5 .. 3)
LIGHT_SETS = ("point", "direction", "four")


def phong_points(s, winner=None, y0=0, y1=None):
    """(ys, xs, t, pt [N, 3], inside [N]) of the covered pixels: the surface point of crender_phong.h, restated from
    the host model's own barycentrics, and whether the pixel lies inside its winner (false for a NaN)."""
    winner = s.winner if winner is None else winner
    ys, xs, t, b, z = phong_ref.surface_point(winner, s.tri, P, y0, y1)
    with np.errstate(all="ignore"):
        q = [b[k] / z[:, k] for k in range(3)]
        sm = (q[0] + q[1]) + q[2]
        c = s.tri[t]
        pt = np.stack([((c[:, 0, a] * q[0] + c[:, 1, a] * q[1]) + c[:, 2, a] * q[2]) / sm for a in range(3)], 1)
        b = np.stack(b)
        inside = ((b >= 0) & (b <= 1)).all(0)
    return ys, xs, t, pt, inside


def light_sets(s, corner):
    """The three light sets of the Phong pass: one point, one direction (both run the instance without the loop
    frame) and four: a point, a direction, a point exactly on `corner` — a corner of a triangle that a pixel shows so
    near that corner that the length of the vector to the light is 0 and its unit vector n / 0 or 0 / 0 — and the origin, where L = V at
    every pixel, with kd = ks = 0.  (`corner` None: a corner of the first triangle.)"""
    corner = s.tri[0, 0] if corner is None else corner
    return {"point": [dict(position=POINT, diffuse=0.9, specular=0.5)],
            "direction": [dict(direction=LIGHT, diffuse=0.9, specular=0.5)],
            "four": [dict(position=POINT, diffuse=0.6, specular=0.5), dict(direction=LIGHT, diffuse=0.3, specular=0.25),
                     dict(position=tuple(float(v) for v in corner), diffuse=0.5, specular=0.125),
                     dict(position=(0.0, 0.0, 0.0), diffuse=0.0, specular=0.0)]}


def _lit(s, seed):
    """The z plane of the occlusion pass — view depths around 1 with a relief of +-3 pixel widths, stored as
    z = P[2, 2] + P[3, 2] / zv, about 8 % of it NaN, infinite, P[2, 2] itself (zv is a division by zero) or 1e6 —
    its radius of 6 pixel widths (and of 64 for the halo of 32 px, whose corners lie 50 widths away) and the light
    sets of the Phong pass."""
    rng = np.random.default_rng(seed)
    d = np.float32
    c = ao_ref.constants(P, s.W, s.H, 1.0, 1)
    s.px = float(min(abs(c[2]), abs(c[3])))                   # (pixels are oblong where the frame is)
    zv = (1.0 + s.px * rng.uniform(-3, 3, (s.H, s.W))).astype(d)
    z = (d(P[2, 2]) + d(P[3, 2]) / zv).astype(d)
    odd = rng.uniform(size=z.shape) < 0.08
    z[odd] = rng.choice(d([np.nan, np.inf, -np.inf, P[2, 2], 1e6]), int(odd.sum()))
    s.z = z
    s.ao_radius, s.halo_radius = 6 * s.px, 64 * s.px
    # the first pixel, in row order, whose point is so near a corner of its winner that the length of the vector to it
    # is 0 (the corners of "z_low" at 1e-38: the squares underflow); none on a scene without such a triangle
    ys, xs, t, pt, _ = phong_points(s)
    with np.errstate(all="ignore"):
        lv = s.tri[t] - pt[:, None, :]
        ll = np.sqrt((lv[..., 0] * lv[..., 0] + lv[..., 1] * lv[..., 1]) + lv[..., 2] * lv[..., 2])
    at, corner = np.nonzero(ll == 0)
    s.on_corner = (int(t[at[0]]), int(corner[0])) if len(at) else None
    s.lights = light_sets(s, s.tri[s.on_corner] if len(at) else None)
    return s


# ---- what the two wire passes need: drawn after everything above, from generators of their own -----------------------

SPARSE_H, SPARSE_W = 97, 101          # the outline's tiles of 32: three whole ones each way, then one row and five columns
TILE = 32
SPARSE_COLUMNS = (0, 31, 32, 63, 64, 95, 96, 100)
SPARSE_RADII = (1, 8)
SPARSE_STRIP = (37, 75)               # rows of the strip frame: neither end a multiple of 32


def _wired(s, seed, z=False):
    """An edge mask in the caller's order, bits 3 to 7 set at random (they are ignored); with `z` a z plane for a scene
    that has none (the tall frame): projected depths of the range its triangles have, a tenth of it NaN or infinite."""
    rng = np.random.default_rng(seed)
    s.edges = rng.integers(0, 256, s.T).astype(np.uint8)
    if z:
        plane = rng.uniform(0.4, 1.0, (s.H, s.W)).astype(np.float32)
        odd = rng.uniform(size=plane.shape) < 0.1
        plane[odd] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 1e6]), int(odd.sum()))
        s.z = plane
    return s


# ---- the tie of the hidden-line test, the clamp of s and the depth ze: two triangles and a degenerate third ----------

TIE_H, TIE_W, TIE_RADIUS, TIE_BIAS = 40, 40, 3, 1e-3
TIE_A, TIE_B, TIE_A2 = 0, 1, 2
TIE_KINDS = ("exact", "above", "below")


def tie_operands(proj, t, e, xs, ys, bias=TIE_BIAS):
    """(s before the clamp, s, d, ze, ze - bias) of crender_wire_outline's "Per edge" for edge e of triangle t at the
    pixels (xs, ys): the model's own float32 statements (tests/outline_ref.py), one operation per step."""
    d_ = np.float32
    a, b = proj[t, e], proj[t, (e + 1) % 3]
    fx, fy = xs.astype(d_), ys.astype(d_)
    with np.errstate(all="ignore"):
        ex, ey = b[0] - a[0], b[1] - a[1]
        px, py = fx - a[0], fy - a[1]
        raw = (px * ex + py * ey) / (ex * ex + ey * ey)
        s = np.where(raw < 0, d_(0), raw)
        s = np.where(s > 1, d_(1), s)
        qx, qy = a[0] + s * ex, a[1] + s * ey
        cx, cy = fx - qx, fy - qy
        d = np.sqrt(cx * cx + cy * cy)
        ze = a[2] + s * (b[2] - a[2])
        return raw, s, d, ze, ze - d_(np.float32(bias))


def near(mask, radius):
    """The pixels within `radius` (in both coordinates) of a pixel of `mask`."""
    h, w = mask.shape
    pad = np.zeros((h + 2 * radius, w + 2 * radius), bool)
    pad[radius:radius + h, radius:radius + w] = mask
    out = np.zeros_like(mask)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


@functools.lru_cache(maxsize=None)
def tie_scene():
    """A near triangle A whose edge 0 alone is drawn, over a far triangle B that covers the frame and draws nothing; A2,
    a copy of A whose edge 0 has no length (s is 0 / 0), painted as a small patch of its own.  The winner plane is
    painted: A's pixels are those inside it, so that B's pixels within TIE_RADIUS of them lie along the drawn edge
    (0 <= s <= 1), beyond its two ends (s < 0, s > 1) and around the two other edges.  At those pixels the window holds
    A and B only and whether A's edge counts is a function of one (t, e): d_z[p] there is, by the residue of x + 2 y,
    exactly ze - depth_bias (computed with the model's statements for that pixel), one ulp above it or one below — the
    scheme of the shadow map in `_build`."""
    d = np.float32
    s = Scene()
    s.H, s.W, s.T = TIE_H, TIE_W, 3
    corners = np.float64([(12.3, 9.6), (25.7, 14.2), (15.1, 27.4)])
    zs = [1.0, 1.3, 1.15]
    A = unproject(corners[:, 0], corners[:, 1], zs, TIE_W, TIE_H)
    B = unproject(np.float64([-10, 100, -10]), np.float64([-10, -10, 100]), 2.0, TIE_W, TIE_H)
    A2 = A.copy()
    A2[1] = A2[0]
    s.tri = np.ascontiguousarray(np.stack([A, B, A2]), np.float32)
    s.edges = np.uint8([1, 0, 1])
    ys, xs = np.mgrid[0:TIE_H, 0:TIE_W]
    inside = np.ones((TIE_H, TIE_W), bool)
    for k in range(3):                                         # (painted: any rule will do, this one is exact in float64)
        (ax, ay), (bx, by) = corners[k], corners[(k + 1) % 3]
        inside &= (bx - ax) * (ys - ay) - (by - ay) * (xs - ax) >= 0
    winner = np.full((TIE_H, TIE_W), TIE_B, np.int32)
    winner[inside] = TIE_A
    winner[32:37, 31:36] = TIE_A2
    s.winner = winner
    s.is_a, s.is_a2 = winner == TIE_A, winner == TIE_A2
    assert not (near(s.is_a, 2 * TIE_RADIUS + 1) & s.is_a2).any()        # no window holds both
    s.ring = (winner == TIE_B) & near(s.is_a, TIE_RADIUS)
    s.ring2 = (winner == TIE_B) & near(s.is_a2, TIE_RADIUS)
    rng = np.random.default_rng(20249)
    s.color = rng.uniform(0, 255, (TIE_H, TIE_W, 3)).astype(d)
    z = np.full((TIE_H, TIE_W), d(0.875), d)                   # B's own projected depth; A's pixels never ask
    s.proj = tex_ref.project(s.tri, P, TIE_W, TIE_H)
    ry, rx = np.nonzero(s.ring)
    at = tie_operands(s.proj, TIE_A, 0, rx, ry)[4]
    kind = (rx + 2 * ry) % 3
    up, down = np.nextafter(at, d(np.inf), dtype=d), np.nextafter(at, d(-np.inf), dtype=d)
    z[ry, rx] = np.where(kind == 0, at, np.where(kind == 1, up, down))
    s.z = z
    s.kind = np.full((TIE_H, TIE_W), -1)
    s.kind[ry, rx] = kind
    return s


# ---- lone winners on a frame of background: the rows a wavefront of the outline skips, and the seams of its tiles ----

def _lone_triangle(x, y, direction):
    """A triangle with edge 0 through the pixel (x, y), a quarter of a pixel off its centre and 100 px long both ways:
    vertical ("v": the pixels above and below in column x are 0.25 px from it) or horizontal ("h")."""
    if direction == "v":
        pts = [(x + 0.25, y - 100), (x + 0.25, y + 100), (x + 50, y)]
    else:
        pts = [(x - 100, y + 0.25), (x + 100, y + 0.25), (x, y + 50)]
    pts = np.float64(pts)
    return unproject(pts[:, 0], pts[:, 1], 1.0, SPARSE_W, SPARSE_H)


def tiles_that_stage(x, radius):
    """The tile columns (or rows) whose staged span, the tile and `radius` of halo either side, holds coordinate x."""
    return {k for k in range(-(-max(SPARSE_H, SPARSE_W) // TILE)) if k * TILE - radius <= x < (k + 1) * TILE + radius}


def sparse_winners():
    """[(x, y, direction)]: a "v" winner at every row 0 .. 96 and an "h" winner at every one of SPARSE_COLUMNS.  The
    columns of the "v" winners: an even row takes one staged by the two left tile columns alone, the odd row after it one
    that no tile stages together with it (the two share a frame); in the first tile row both lie just left of a seam."""
    out = []
    for y in range(SPARSE_H):
        ty, k = y // TILE, (y // 2) % 2
        if y % 2 == 0:
            x = (31, 0, 32, 0)[ty]
        else:
            x = (95, (64, 63)[k], (100, 96)[k])[ty]
        out.append((x, y, "v"))
    for k, x in enumerate(SPARSE_COLUMNS):
        out.append((x, (7 + 23 * k) % SPARSE_H, "h"))
    return out


@functools.lru_cache(maxsize=None)
def sparse_frames(radius):
    """The lone winners of `sparse_winners` packed into frames, first fit: two winners share a frame only if no tile
    stages both or their rows are 2 radius + 2 or more apart — the rows a wavefront of k_wire_outline reaches, its own
    two and `radius` either side, then hold at most one winner, and no pixel sees two.  Each frame: a Scene with
    tri [T, 3, 3], edges (edge 0 alone), winner, z, colour and `lone`, the [(x, y, direction)] of triangles 0 .. T - 1."""
    frames = []
    span = 2 * radius + 2                                      # ("v" rows a span apart, and each with the next row, first)
    for x, y, direction in sorted(sparse_winners(), key=lambda w: (w[2] == "h", w[1] % span // 2, w[1])):
        cols = tiles_that_stage(x, radius)
        for lone in frames:
            if all(abs(y - y2) >= span or not (cols & tiles_that_stage(x2, radius)) for x2, y2, _ in lone):
                lone.append((x, y, direction))
                break
        else:
            frames.append([(x, y, direction)])
    return [_sparse_scene(lone, 20250 + 100 * radius + k) for k, lone in enumerate(frames)]


def _sparse_scene(lone, seed):
    rng = np.random.default_rng(seed)
    s = Scene()
    s.H, s.W, s.T, s.lone = SPARSE_H, SPARSE_W, len(lone), list(lone)
    s.tri = np.ascontiguousarray(np.stack([_lone_triangle(*w) for w in lone]), np.float32)
    s.edges = np.full(s.T, 1, np.uint8)
    s.winner = np.full((SPARSE_H, SPARSE_W), -1, np.int32)
    for t, (x, y, _) in enumerate(lone):
        s.winner[y, x] = t
    s.z = rng.uniform(0.4, 1.0, (SPARSE_H, SPARSE_W)).astype(np.float32)
    s.color = rng.uniform(0, 255, (SPARSE_H, SPARSE_W, 3)).astype(np.float32)
    return s


def extreme_taps(s, radius):
    """[(t, x, y, px, py)]: for every lone winner t at (x, y) of a sparse frame, the in-frame pixels (px, py) exactly
    `radius` rows ("v") or columns ("h") from it, both signs, in the winner's own column (row) and in the next one:
    0.25 px and 0.75 px from the edge, on a line of width 1 and feather 1 both."""
    out = []
    for t, (x, y, direction) in enumerate(s.lone):
        for sign in (-1, 1):
            for side in (0, 1):
                px, py = (x + side, y + sign * radius) if direction == "v" else (x + sign * radius, y + side)
                if 0 <= px < s.W and 0 <= py < s.H:
                    out.append((t, x, y, px, py))
    return out


@functools.lru_cache(maxsize=None)
def sparse_strip():
    """A frame for the rows SPARSE_STRIP: lone "v" winners on the row above the strip and on the first row below it,
    whose lines would cross the strip's outermost rows, and one inside it, which the pass does see."""
    y0, y1 = SPARSE_STRIP
    return _sparse_scene([(20, y0 - 1, "v"), (70, y1, "v"), (45, (y0 + y1) // 2, "v")], 20259)


def outline_model(s, winner=None, edges=None, field=None, **kw):
    """tests/outline_ref.py's wire_pass on a scene's own planes."""
    return outline_ref.wire_pass(s.color, s.winner if winner is None else winner, s.z, s.tri, P, edges=edges, field=field, **kw)
