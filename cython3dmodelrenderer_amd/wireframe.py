"""Which edges of a mesh a wireframe should show: the per-triangle edge masks ``AdvancedPixelBufferFiller.wire_pass``
takes as ``edges``.  Host numpy in float64, once per model: not a hot path."""
import numpy as np


def feature_edges(vertices_by_triangles, angle=30.0):
    """uint8 [T]: bit e of entry t is set if the edge of triangle t from corner e to corner (e + 1) % 3 is a feature
    edge of the mesh `vertices_by_triangles` (float32 [T, 3, 3], ``Model._vertices_by_triangles``).

    Two triangle edges are the same edge when their two end points have the same float32 bit patterns, as an
    unordered pair.  An edge is a feature, in every triangle that has it, if it has no partner (a border), more than
    one partner, a face without area at either side, or if the angle between the two faces' geometric normals (from
    the winding, as the corners are given) exceeds `angle` degrees.  The diagonal of a flat quad is none at any
    `angle` >= 0: the angle between two equal normals is exactly 0."""
    tri = np.ascontiguousarray(vertices_by_triangles, np.float32)
    if tri.ndim != 3 or tri.shape[1:] != (3, 3):
        raise ValueError(f"vertices_by_triangles must have shape [T, 3, 3], got {tuple(tri.shape)}")
    T = tri.shape[0]
    if T == 0:
        return np.zeros(0, np.uint8)
    # half-edge h = 3 t + e; its end points as bit patterns, the smaller one (lexicographically) first
    bits = tri.view(np.uint32).astype(np.uint64)
    a, b = bits.reshape(-1, 3), bits[:, [1, 2, 0]].reshape(-1, 3)
    swap = np.zeros(3 * T, bool)
    for c in (2, 1, 0):                      # the last pass decides: coordinate 0 first
        swap = np.where(a[:, c] != b[:, c], a[:, c] > b[:, c], swap)
    lo, hi = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
    keys = np.concatenate([lo, hi], 1)
    order = np.lexsort(keys.T[::-1])         # one sort of the edge keys
    sk = keys[order]
    first = np.ones(3 * T, bool)
    first[1:] = (sk[1:] != sk[:-1]).any(1)
    group = np.cumsum(first) - 1             # the edge of every sorted half-edge
    size = np.bincount(group)
    # geometric normals in float64
    v = tri.astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    with np.errstate(all="ignore"):
        flat = ~(np.einsum("ij,ij->i", n, n) > 0)      # no area (or not finite)
        feature = size[group] != 2                     # borders, and edges of three or more faces
        pair = np.nonzero(first & (size[group] == 2))[0]
        t0, t1 = order[pair] // 3, order[pair + 1] // 3
        n0, n1 = n[t0], n[t1]
        c = np.cross(n0, n1)
        theta = np.degrees(np.arctan2(np.sqrt(np.einsum("ij,ij->i", c, c)), np.einsum("ij,ij->i", n0, n1)))
        crease = flat[t0] | flat[t1] | ~(theta <= float(angle))
    feature[pair] = crease
    feature[pair + 1] = crease
    drawn = np.zeros(3 * T, bool)
    drawn[order] = feature
    return (drawn.reshape(T, 3) * np.uint8([1, 2, 4])).sum(1).astype(np.uint8)
