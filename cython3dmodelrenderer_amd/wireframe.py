"""Which edges of a mesh a wireframe should show: the per-triangle edge masks ``AdvancedPixelBufferFiller.wire_pass``
takes as ``edges`` (``feature_edges``: creases and borders), and the mesh's connectivity as the table from which
``AdvancedPixelBufferFiller.contour_edges`` classifies the edges of a view on the device (``edge_partners``).  Host numpy
in float64, or torch ops on the device the triangles are on; once per model: not a hot path."""
import numpy as np


def _triangles(vertices_by_triangles):
    tri = np.ascontiguousarray(vertices_by_triangles, np.float32)
    if tri.ndim != 3 or tri.shape[1:] != (3, 3):
        raise ValueError(f"vertices_by_triangles must have shape [T, 3, 3], got {tuple(tri.shape)}")
    return tri


def _edge_groups(tri):
    """The one sort of the half-edges of `tri` (float32 [T, 3, 3], T > 0) by their edge: (order, first, group, size,
    swap).  Half-edge h = 3 t + e; ``order`` lists the half-edges edge by edge, ``first`` marks the first one of every
    edge in that list, ``group`` numbers the edge of every listed half-edge and ``size`` counts the half-edges of every
    edge.  ``swap[h]`` (in h's own order): the first end point of h is the greater one."""
    T = tri.shape[0]
    # its end points as bit patterns, the smaller one (lexicographically) first
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
    return order, first, group, size, swap


def feature_edges(vertices_by_triangles, angle=30.0):
    """uint8 [T]: bit e of entry t is set if the edge of triangle t from corner e to corner (e + 1) % 3 is a feature
    edge of the mesh `vertices_by_triangles` (float32 [T, 3, 3], ``Model._vertices_by_triangles``).

    Two triangle edges are the same edge when their two end points have the same float32 bit patterns, as an
    unordered pair.  An edge is a feature, in every triangle that has it, if it has no partner (a border), more than
    one partner, a face without area at either side, or if the angle between the two faces' geometric normals (from
    the winding, as the corners are given) exceeds `angle` degrees.  The diagonal of a flat quad is none at any
    `angle` >= 0: the angle between two equal normals is exactly 0."""
    tri = _triangles(vertices_by_triangles)
    T = tri.shape[0]
    if T == 0:
        return np.zeros(0, np.uint8)
    order, first, group, size, _ = _edge_groups(tri)
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


MAX_TRIANGLES = 1 << 30            # an entry 2 p + s of the partner table is an int32


def edge_partners(vertices_by_triangles):
    """int32 [T, 3]: the partner table of the mesh `vertices_by_triangles` (float32 [T, 3, 3]), what
    ``AdvancedPixelBufferFiller.contour_edges`` takes (``crender_wire_contours``, include/crender_wire.h).  A numpy array
    gives a numpy array; a torch tensor gives a tensor on its device, made there with torch's sort and unique: nothing
    is downloaded.  The two forms return equal tables.

    Edges are ``feature_edges``' edges: two half-edges are the same edge when their end points have the same float32
    bit patterns, as an unordered pair (-0.0 and +0.0 differ).  Entry [t, e], for the half-edge from corner e to corner
    (e + 1) % 3 of triangle t, is -1 if the edge has no other half-edge (a border), -2 if it has more than one, and
    otherwise ``2 * p + s``: p is the triangle that holds the other half-edge (t itself for a triangle with two equal
    corners), s is 0 if the two run in opposite directions between the two bit patterns (a consistent winding) and 1 if
    they run the same way.  Direction: a half-edge is swapped if its first corner's bit patterns, as unsigned integers
    compared lexicographically from coordinate 0, are greater than its second's; two half-edges run the same way iff
    both are swapped or neither is.  The table does not change when the model is moved as a whole by an operation
    that gives equal vertices equal results (a rotation of shared vertices, a shift): make it once per model."""
    if hasattr(vertices_by_triangles, "data_ptr"):
        return _edge_partners_torch(vertices_by_triangles)
    tri = _triangles(vertices_by_triangles)
    T = tri.shape[0]
    if T >= MAX_TRIANGLES:
        raise ValueError(f"edge_partners takes fewer than 2^30 triangles, got {T}")
    if T == 0:
        return np.zeros((0, 3), np.int32)
    order, first, group, size, swap = _edge_groups(tri)
    sorted_entry = np.where(size[group] == 1, -1, -2).astype(np.int64)
    pair = np.nonzero(first & (size[group] == 2))[0]
    h0, h1 = order[pair], order[pair + 1]
    s = (swap[h0] == swap[h1]).astype(np.int64)
    sorted_entry[pair] = 2 * (h1 // 3) + s
    sorted_entry[pair + 1] = 2 * (h0 // 3) + s
    table = np.empty(3 * T, np.int32)
    table[order] = sorted_entry
    return table.reshape(T, 3)


def _edge_partners_torch(tri):
    """``edge_partners`` with torch ops on the device of `tri`."""
    import torch
    if tri.dtype != torch.float32 or tri.dim() != 3 or tuple(tri.shape[1:]) != (3, 3):
        raise ValueError(f"vertices_by_triangles must be float32 [T, 3, 3], got {tri.dtype} {tuple(tri.shape)}")
    T = tri.shape[0]
    if T >= MAX_TRIANGLES:
        raise ValueError(f"edge_partners takes fewer than 2^30 triangles, got {T}")
    if T == 0:
        return torch.zeros((0, 3), dtype=torch.int32, device=tri.device)
    # the corners as bit patterns, unsigned; a corner's id is its rank among the distinct triples, which unique leaves
    # in lexicographic order: comparing ids is the host's comparison of triples
    bits = (tri.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF).reshape(3 * T, 3)
    ids = torch.unique(bits, dim=0, return_inverse=True)[1].reshape(T, 3)
    a, b = ids.reshape(-1), ids[:, [1, 2, 0]].reshape(-1)
    swap = a > b
    keys = torch.stack([torch.minimum(a, b), torch.maximum(a, b)], 1)
    _, group, size = torch.unique(keys, dim=0, return_inverse=True, return_counts=True)
    order = torch.argsort(group, stable=True)             # the half-edges edge by edge
    n = size[group[order]]                                # the size of every listed half-edge's edge
    entry = torch.where(n == 1, -1, -2).to(torch.int64)
    first = torch.ones(3 * T, dtype=torch.bool, device=tri.device)
    first[1:] = group[order][1:] != group[order][:-1]
    pair = torch.nonzero(first & (n == 2)).reshape(-1)
    h0, h1 = order[pair], order[pair + 1]
    s = (swap[h0] == swap[h1]).to(torch.int64)
    entry[pair] = 2 * torch.div(h1, 3, rounding_mode="floor") + s
    entry[pair + 1] = 2 * torch.div(h0, 3, rounding_mode="floor") + s
    table = torch.empty(3 * T, dtype=torch.int32, device=tri.device)
    table[order] = entry.to(torch.int32)
    return table.reshape(T, 3)
