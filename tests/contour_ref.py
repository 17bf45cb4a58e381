"""Host model of the contour edges: the statements of include/crender_wire.h (crender_wire_contours) in vectorised
numpy, one float32 operation per step, over (the unprojected triangles and projection matrix, the partner table, a static
mask, the flag).  The GPU tests compare csrc/wireframe.hip's k_wire_facing and k_wire_contour_mask with it bit for bit: a
uint8 mask has no tolerance.  tests/test_wire_contours_cpu.py pins it by counts on T-Rex and by identities on generated
meshes.  Also here: the generated meshes the two files share."""
import numpy as np

import tex_ref

BORDERS = 1


def facing(tri, P, W, H, pos_of=None):
    """Phase 1: int8 [T], the sign of every triangle's projected area.  With a `pos_of` (uint32 [T]), `tri` is the
    resident copy and triangle t sits at tri[pos_of[t]]; an entry >= T gives 0."""
    tri = np.ascontiguousarray(tri, np.float32)
    T = tri.shape[0]
    out = np.zeros(T, np.int8)
    if T == 0:
        return out
    q = np.arange(T, dtype=np.int64) if pos_of is None else np.asarray(pos_of).astype(np.uint32).astype(np.int64)
    ok = q < T
    with np.errstate(all="ignore"):
        c = tex_ref.project(tri[q[ok]], P, W, H)
        x0, y0, x1, y1, x2, y2 = c[:, 0, 0], c[:, 0, 1], c[:, 1, 0], c[:, 1, 1], c[:, 2, 0], c[:, 2, 1]
        l1, l2 = x1 - x2, y1 - y2
        A = l1 * (y0 - y2) - l2 * (x0 - x2)
        assert A.dtype == np.float32
        out[ok] = np.where(A > 0, 1, np.where(A < 0, -1, 0)).astype(np.int8)       # (a NaN is neither)
    return out


def contours(face, partners):
    """bool [T, 3]: the half-edges that are contours under the signs `face`."""
    face = np.asarray(face, np.int8).astype(np.int32)
    v = np.asarray(partners, np.int32).astype(np.int64)
    T = face.shape[0]
    assert v.shape == (T, 3)
    p = v >> 1
    ok = (v >= 0) & (p < T)                              # anything else is "no partner": never an index
    other = face[np.where(ok, p, 0)]
    want = np.where(v & 1, 1, -1)
    return ok & (face[:, None] * other == want)


def mask(face, partners, static=None, flags=0):
    """Phase 2: uint8 [T]."""
    v = np.asarray(partners, np.int32)
    on = contours(face, v)
    if flags & BORDERS:
        on |= (v == -1) | (v == -2)
    bits = (on * np.uint8([1, 2, 4])).sum(1).astype(np.uint8)
    if static is not None:
        bits |= np.asarray(static, np.uint8) & np.uint8(7)
    return bits


def contour_edges(tri, P, W, H, partners, static=None, borders=False, pos_of=None):
    """(mask uint8 [T], facing int8 [T]) of crender_wire_contours."""
    f = facing(tri, P, W, H, pos_of)
    return mask(f, partners, static, BORDERS if borders else 0), f


def edge_keys(tri, bits):
    """The set of the edges a mask draws, each as the sorted pair of its end points' bit patterns."""
    u = np.ascontiguousarray(tri, np.float32).view(np.uint32)
    out = set()
    for t, e in zip(*np.nonzero((np.asarray(bits)[:, None] >> np.arange(3)) & 1)):
        a, b = tuple(u[t, e]), tuple(u[t, (e + 1) % 3])
        out.add((min(a, b), max(a, b)))
    return out


# ---- generated meshes: [T, 3, 3] float32 in the camera's frame, in front of it -------------------------------------

CENTRE = (0.0, 0.0, 3.0)


def place(tri, angles=(0.0, 0.0, 0.0), centre=CENTRE):
    """The mesh turned about x, y, z (degrees) and moved to `centre`.  Every vertex goes through the same float64
    statements, so shared vertices stay shared bit for bit."""
    ax, ay, az = np.radians(angles)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    v = np.asarray(tri, np.float32).astype(np.float64) @ (rx @ ry @ rz).T + np.asarray(centre, np.float64)
    return np.ascontiguousarray(v.astype(np.float32))


def uv_sphere(stacks=10, slices=16, radius=1.0):
    """A closed, consistently wound sphere of 2 * slices * (stacks - 1) triangles about the origin."""
    th = np.linspace(0.0, np.pi, stacks + 1)[1:-1]
    ph = np.arange(slices) * (2.0 * np.pi / slices)
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.cos(th)[:, None] * np.ones_like(ph), np.sin(th)[:, None] * np.sin(ph)], 2)
    ring = (radius * ring).astype(np.float32)                                      # [stacks - 1, slices, 3]
    top, bottom = np.float32([0, radius, 0]), np.float32([0, -radius, 0])
    tris = []
    for j in range(slices):
        k = (j + 1) % slices
        tris.append([top, ring[0, k], ring[0, j]])
        tris.append([bottom, ring[-1, j], ring[-1, k]])
        for i in range(stacks - 2):
            tris.append([ring[i, j], ring[i, k], ring[i + 1, j]])
            tris.append([ring[i, k], ring[i + 1, k], ring[i + 1, j]])
    return np.ascontiguousarray(np.float32(tris))


def open_cylinder(rings=4, slices=16, radius=0.8, height=1.6):
    """An open, consistently wound tube of 2 * slices * rings triangles about the origin: two rims of `slices` edges."""
    ph = np.arange(slices) * (2.0 * np.pi / slices)
    ys = np.linspace(-height / 2, height / 2, rings + 1)
    v = np.stack([radius * np.cos(ph)[None, :] * np.ones((rings + 1, 1)), ys[:, None] * np.ones((1, slices)),
                  radius * np.sin(ph)[None, :] * np.ones((rings + 1, 1))], 2).astype(np.float32)
    tris = []
    for i in range(rings):
        for j in range(slices):
            k = (j + 1) % slices
            tris.append([v[i, j], v[i + 1, j], v[i, k]])
            tris.append([v[i, k], v[i + 1, j], v[i + 1, k]])
    return np.ascontiguousarray(np.float32(tris))


def hand_mesh():
    """(tri, its partner table): eight triangles with a consistent pair (on BC), a pair wound alike (on AB), an edge of
    three triangles (CA), borders, a triangle with two equal corners, and two triangles that would share an edge if
    -0.0 were +0.0."""
    A, B, Cc, D = (0, 0, 3), (1, 0, 3), (0, 1, 3), (1, 1, 3)
    E, F, G, Hh = (0.5, -1, 3), (-0.5, 0.5, 2.5), (-0.5, 0.5, 3.5), (2, 1, 3)
    Pp, Pm, Q, R, S = (0.0, 2, 3), (-0.0, 2, 3), (1, 2, 3), (0.5, 3, 3), (0.5, 1.5, 3)
    tri = np.float32([[A, B, Cc], [B, D, Cc], [A, B, E], [Cc, A, F], [A, Cc, G], [D, D, Hh], [Pp, Q, R], [Q, Pm, S]])
    assert np.signbit(tri[7, 1, 0]) and not np.signbit(tri[6, 0, 0])
    want = np.int32([[2 * 2 + 1, 2 * 1 + 0, -2], [-1, -1, 2 * 0 + 0], [2 * 0 + 1, -1, -1], [-2, -1, -1], [-2, -1, -1],
                     [-1, 2 * 5 + 0, 2 * 5 + 0], [-1, -1, -1], [-1, -1, -1]])
    return np.ascontiguousarray(tri), want


def sphere_model(stacks=10, slices=16):
    """The sphere as an indexed ``Model`` (shared vertices, recalculated normals, one colour) about CENTRE."""
    from cython3dmodelrenderer_amd.data_structures.model import Model
    tri = uv_sphere(stacks, slices)
    vertices, faces = np.unique(tri.reshape(-1, 3), axis=0, return_inverse=True)
    m = Model(vertices + np.float32(CENTRE), faces.reshape(-1, 3).astype(np.int32))
    m.set_uniform_color((200.0, 180.0, 160.0))
    return m


def attributes(tri, seed=0):
    """(colours, normals) to render `tri` with: random colours, every normal towards the camera (none is culled)."""
    col = np.random.default_rng(seed).uniform(30.0, 255.0, tri.shape).astype(np.float32)
    nrm = np.zeros_like(tri)
    nrm[..., 2] = -1.0
    return col, nrm
