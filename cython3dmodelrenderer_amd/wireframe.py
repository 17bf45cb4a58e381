"""Which edges of a mesh a wireframe should show: the per-triangle edge masks ``AdvancedPixelBufferFiller.wire_pass``
takes as ``edges`` (``feature_edges``: creases and borders), and the mesh's connectivity as the table from which
``AdvancedPixelBufferFiller.contour_edges`` classifies the edges of a view on the device (``edge_partners``).  Host numpy
in float64, or torch ops on the device the triangles are on; once per model: not a hot path.  And for the drawing as
vectors (``AdvancedPixelBufferFiller.line_runs``): ``half_edges_once``, which leaves one half-edge of every drawn edge in
a mask, and ``write_svg``, which writes the runs out."""
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


def half_edges_once(edges, partners):
    """uint8 [T]: the edge mask `edges` (uint8 [T], or None for every edge) with one of the two half-edges of every drawn
    mesh edge cleared, so that ``AdvancedPixelBufferFiller.line_runs`` walks every drawn edge exactly once.  `partners` is
    the mesh's partner table (int32 [T, 3], ``edge_partners``).  numpy arrays give a numpy array; torch tensors give a
    tensor on the device of `partners`, made there: nothing is downloaded.

    Bit e of triangle i is cleared when it is set, ``partners[i, e] >= 0``, the partner ``p = partners[i, e] >> 1`` is
    below i, and some half-edge e' of p names i as its partner (``partners[p, e'] >= 0`` and ``partners[p, e'] >> 1 ==
    i``) and is drawn itself.  Borders, edges of more than two faces, the half-edge of the smaller triangle and every
    half-edge whose twin is not drawn stay.  Bits 3 to 7 come out 0.  Applying it twice changes nothing more."""
    if hasattr(partners, "data_ptr"):
        import torch
        T = partners.shape[0]
        if partners.dtype != torch.int32 or partners.dim() != 2 or partners.shape[1] != 3:
            raise ValueError(f"partners must be int32 [T, 3] (edge_partners), got {partners.dtype} {tuple(partners.shape)}")
        ids = torch.arange(T, device=partners.device)
        shifts = torch.arange(3, device=partners.device)
        weights = torch.tensor([1, 2, 4], device=partners.device)
        if edges is None:
            bits = torch.full((T,), 7, dtype=torch.int64, device=partners.device)
        else:
            if not hasattr(edges, "data_ptr"):
                edges = torch.from_numpy(np.ascontiguousarray(edges))
            if edges.dtype != torch.uint8 or tuple(edges.shape) != (T,):
                raise ValueError(f"edges must be uint8 [T] with T = {T}, got {edges.dtype} {tuple(edges.shape)}")
            bits = edges.to(partners.device).to(torch.int64)
        table = partners.to(torch.int64)
        clip = lambda a: a.clamp(0, max(T - 1, 0))      # noqa: E731
        as_u8 = lambda a: a.to(torch.uint8)             # noqa: E731
    else:
        table = np.asarray(partners)
        if table.dtype != np.int32 or table.ndim != 2 or table.shape[1] != 3:
            raise ValueError(f"partners must be int32 [T, 3] (edge_partners), got {table.dtype} {tuple(table.shape)}")
        T = table.shape[0]
        ids, shifts, weights = np.arange(T), np.arange(3), np.array([1, 2, 4])
        if edges is None:
            bits = np.full(T, 7, np.int64)
        else:
            given = np.asarray(edges)
            if given.dtype != np.uint8 or given.shape != (T,):
                raise ValueError(f"edges must be uint8 [T] with T = {T}, got {given.dtype} {tuple(given.shape)}")
            bits = given.astype(np.int64)
        table = table.astype(np.int64)
        clip = lambda a: np.clip(a, 0, max(T - 1, 0))   # noqa: E731
        as_u8 = lambda a: a.astype(np.uint8)            # noqa: E731
    if T == 0:
        return as_u8(bits)
    drawn = ((bits[:, None] >> shifts[None, :]) & 1) == 1                      # [T, 3]
    p = table >> 1
    lower = drawn & (table >= 0) & (p < ids[:, None])
    back = table[clip(p)]                                                     # [T, 3, 3]: the partner's own row
    twin = ((back >= 0) & ((back >> 1) == ids[:, None, None]) & drawn[clip(p)]).any(-1)
    keep = drawn & ~(lower & twin)
    return as_u8((keep * weights[None, :]).sum(1))


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def write_svg(target, drawing, stroke="#000", width=1.0, hidden=True, hidden_dash=(4, 4), hidden_opacity=0.5,
              background=None, scale=1.0):
    """Write the ``LineDrawing`` of ``AdvancedPixelBufferFiller.line_runs`` as an SVG to `target`, a path or a text file
    object.  Host code on the standard library: one download of ``drawing.ends`` and one of the classes.

    The centre of pixel (x, y) maps to ((x + 0.5) * scale, (y + 0.5) * scale), computed in double precision from the float32
    coordinates, and the picture is ``width * scale`` by ``height * scale`` of the drawing's frame.  Every run is one
    ``<line>``: the hidden runs in a group ``class="hidden"`` with ``stroke-dasharray`` `hidden_dash` and
    ``stroke-opacity`` `hidden_opacity` (left out with ``hidden=False``), then the visible runs, solid, in a group
    ``class="visible"``, which so paints over the hidden one.  `stroke` and `width` (in SVG units, not scaled) are both
    groups'; `background`, a colour, puts a rectangle under everything.  Coordinates are written with three decimals
    (``"%.3f"``): equal float32 coordinates give equal text, so chains of edges that share an end point close exactly."""
    from xml.sax.saxutils import quoteattr
    ends = _host(drawing.ends).astype(np.float64)
    cls = _host(drawing.runs[:, 3])
    scale = float(scale)
    if not scale > 0 or not np.isfinite(scale):
        raise ValueError(f"scale must be a positive number, got {scale!r}")
    on, off = (float(v) for v in hidden_dash)
    W, H = drawing.width * scale, drawing.height * scale
    out = ['<?xml version="1.0" encoding="UTF-8"?>\n',
           f'<svg xmlns="http://www.w3.org/2000/svg" version="1.1" width="{W:.3f}" height="{H:.3f}" '
           f'viewBox="0 0 {W:.3f} {H:.3f}">\n']
    if background is not None:
        out.append(f'<rect x="0" y="0" width="{W:.3f}" height="{H:.3f}" fill={quoteattr(str(background))}/>\n')
    xy = (ends + 0.5) * scale
    style = f'fill="none" stroke={quoteattr(str(stroke))} stroke-width="{float(width):g}"'
    groups = [("visible", 2, ' stroke-linecap="round"')]
    if hidden:
        groups.insert(0, ("hidden", 1, f' stroke-linecap="butt" stroke-opacity="{float(hidden_opacity):g}" '
                                       f'stroke-dasharray="{on:g},{off:g}"'))
    for name, value, more in groups:
        out.append(f'<g class="{name}" {style}{more}>\n')
        for x0, y0, x1, y1 in xy[cls == value].tolist():
            out.append(f'<line x1="{x0:.3f}" y1="{y0:.3f}" x2="{x1:.3f}" y2="{y1:.3f}"/>\n')
        out.append("</g>\n")
    out.append("</svg>\n")
    text = "".join(out)
    if hasattr(target, "write"):
        target.write(text)
    else:
        with open(target, "w", encoding="utf-8") as fh:
            fh.write(text)
