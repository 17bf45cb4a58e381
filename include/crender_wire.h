/*
 * crender_wire.h — C ABI of the wireframe filler (EdgeOnlyPixelBufferFiller) of
 * libcrender_hip.so, and of the hidden-line overlay over AdvancedPixelBufferFiller's winner plane
 * (crender_wire_overlay, and crender_wire_outline for lines at full width, at the end; crender_wire_contours picks the edges
 * of a view for both, crender_wire_hidden draws the edges behind the surface, dashed).  Same conventions as crender_hip.h: raw device pointers, an int
 * status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work enqueued
 * on `stream` and nothing synchronised.  Reference files cited below are in the
 * reference's crender/py/ (the crender/cy/ copies are identical but for one import).
 *
 * Result contract: after crender_wire_draw the colour plane holds, bit for bit, what the
 * reference's EdgeOnlyPixelBufferFiller.compute_triangle_statistics leaves when the py
 * Renderer feeds it the triangles in index order (renderer.py:52-59):
 *   - vertex v of triangle i is p_v = (int(tri[i][v][0]), int(tri[i][v][1])), truncated
 *     toward zero, with no projection (edge_only_pixel_buffer_filler.py:16-20);
 *   - edges: the lines p0->p1, p1->p2, p2->p0 of LineBresenham.draw_line
 *     (line_bresenham.py:6-45: float error term el / 2, ties dx == dy on the y-major
 *     branch, el + 1 pixels with the start pixel); dots (CRENDER_WIRE_DOTS): the pixels
 *     p0, p1, p2;
 *   - a pixel outside 0 <= x < W, 0 <= y < H is dropped (buffer.py:66-69);
 *   - colour: line_bgr3, or with CRENDER_WIRE_FORCE_COLORS colors[i][e] for edge / vertex e;
 *     a pixel keeps the colour of its LAST write in the order (triangle i, edge e).
 * Pixel t of a line from (x1, y1) with major length el and minor length es is the major
 * coordinate advanced by t and the minor one by k(t) = ceil((2 t es - el) / (2 el)) (k = 0 for
 * el = 0): the float loop is exact integer arithmetic, so every pixel is computed on its own.
 *
 * Domain: exact for |int(c)| < 2^30 (2 t es then fits in int64).  A NaN, an infinity or any x / y
 * coordinate with |c| >= 2^30 (the reference raises on the first two, after drawing the triangles
 * before it, and loops for ages on the last) sets *d_status to 1 and the call draws NOTHING: the
 * buffers keep their contents, CRENDER_WIRE_CLEAR included.  *d_status is 0 otherwise.  The z and
 * normal planes are never read or written but by CRENDER_WIRE_CLEAR.
 */
#ifndef CRENDER_WIRE_H
#define CRENDER_WIRE_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of crender_wire_draw */
enum {
    CRENDER_WIRE_DOTS = 1u,          /* draw_edges=False: the three vertices, not the three edges   */
    CRENDER_WIRE_FORCE_COLORS = 2u,  /* force_triangle_colors=True: colour of edge / vertex e is
                                      * d_col[i][e]; needs d_col, d_key and T < 2^30                 */
    CRENDER_WIRE_CLEAR = 4u          /* first set z = 1e6, colour = normal = 0 (the initial state of
                                      * the fillers), in the same call and under the same domain check */
};

/* Bytes of the key plane CRENDER_WIRE_FORCE_COLORS needs: uint32 [H][W], zero before the first call
 * and left zero by every call (the draw resolves the last writer of each pixel through it and writes
 * back 0 where it stored).  0 for a bad size. */
CRENDER_API size_t crender_wire_key_bytes(int H, int W);

/* Draw the wireframe of T triangles onto the colour plane d_color float32 [H][W][3].
 *   d_tri     float32 [T][3][3] (only x and y are read)
 *   d_col     float32 [T][3][3] or NULL without CRENDER_WIRE_FORCE_COLORS
 *   line_bgr3 HOST float[3]: the constant colour (unused with CRENDER_WIRE_FORCE_COLORS)
 *   d_z, d_normal  float32 [H][W] and [H][W][3]; only CRENDER_WIRE_CLEAR touches them (may be NULL
 *                  without it)
 *   d_key     uint32 [H][W] of crender_wire_key_bytes, or NULL without CRENDER_WIRE_FORCE_COLORS
 *   d_status  DEVICE int32 [1]: 0, or 1 if an input coordinate is out of the domain (nothing drawn)
 * 1 <= H, W <= 2^20.  Three to five launches; no synchronisation. */
CRENDER_API int crender_wire_draw(const float *d_tri, const float *d_col, int64_t T, const float *line_bgr3,
                                  float *d_z, float *d_color, float *d_normal, uint32_t *d_key, int H, int W,
                                  unsigned flags, int32_t *d_status, void *stream);

/*
 * The hidden-line overlay: a deferred pass over the winner plane a raster launch left (crender_render_model with a
 * d_winner), as crender_phong_shade is.  It draws the edges of every triangle on the pixels that triangle WON, so a
 * line behind a nearer triangle is never drawn: hidden-line removal without a depth bias.
 *
 * Result contract.  For every pixel (x, y) with y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square root (no
 *                contraction into fused multiply-adds, no reciprocal, denormals kept).
 *   Background   t < 0, t >= T, or d_pos_of[t] >= T: the pixel is not written.  Nothing is ever read out of bounds,
 *                whatever the winner plane holds.
 *   Corners      the three vertices of triangle t -- d_tri[t], or d_tri[d_pos_of[t]] with a d_pos_of -- projected as
 *                crender_project projects them (.pyx:116-130): (x_k, y_k), k = 0, 1, 2.
 *   Edge mask    bits = d_edges[t] (indexed by t itself, the caller's order, whatever d_pos_of says), or 7 without
 *                d_edges.  Bit e draws edge e, from corner e to corner (e + 1) % 3: p0->p1, p1->p2, p2->p0, the
 *                numbering of crender_wire_draw's lines.  Bits 3 to 7 are ignored.
 *   Per edge     fx = (float)x, fy = (float)y, m = +inf; for e = 0, 1, 2 in order, if bit e is set, with a = corner e
 *                and b = corner (e + 1) % 3:
 *                  l1 = xa - xb,   l2 = ya - yb
 *                  n  = l1 * (fy - yb) - l2 * (fx - xb)      (the numerator of the barycentric b3, b1, b2 of
 *                                                             math_utils.pyx:8-34 for e = 0, 1, 2)
 *                  len = sqrtf(l1 * l1 + l2 * l2)
 *                  d  = fabsf(n) / len
 *                  if (d < m) m = d
 *                The distance is to the edge's LINE, not to its segment.  A NaN (an edge of no length, a NaN or
 *                infinite corner) is never taken.
 *   Window       hi = width * 0.5f + feather * 0.5f (once, on the host, in float32);
 *                  a  = (hi - m) / feather
 *                  on = a > 0                                 (false for a NaN and for m = +inf)
 *                  a  = a > 1 ? 1 : a
 *                  a  = a * opacity
 *                A pixel within (width - feather) / 2 of a line gets all of `opacity`, one beyond
 *                (width + feather) / 2 none; the ramp between them is linear.
 *   Colour       base = fill3 if given, else the pixel's own colour.  If on, per channel j:
 *                  k = 1.0f - a,   colour_j = base_j * k + line3_j * a
 *                If not on: the pixel is stored with fill3 if it is given, and otherwise NOT written: it keeps its
 *                bits.  With finite colours no NaN reaches a pixel that is on or filled.
 *   Other planes z, normals and the winner plane are only read.
 *
 * Only the winner's side of an edge draws it: the line of a silhouette or border edge is width / 2 wide.  Widths are
 * in pixels; no dashes, no fading with depth.
 */
#define CRENDER_WIRE_MAX_WIDTH 64

/* Overlay the colour plane d_color float32 [H][W][3] over rows y0 <= y < y1.
 *   d_winner   int32 [H][W]: the caller's index of the triangle whose fragment won, -1 = background
 *   d_tri      float32 [T][3][3], UNPROJECTED camera-frame vertices (may be NULL if T == 0)
 *   d_pos_of   NULL, or uint32 [T]: triangle t sits at d_tri[d_pos_of[t]] (the tile-coherent copy of
 *              crender_plan_set_triangle_order); an entry >= T makes t background
 *   P16        HOST float[16], the camera's projection matrix (crender_projection_matrix)
 *   d_edges    NULL (all three edges of every triangle), or uint8 [T] in the CALLER's triangle order
 *   line3      HOST float[3], the colour of the lines
 *   fill3      NULL, or HOST float[3]: the colour every covered pixel is given under the lines (a hidden-line drawing)
 *   width      of a line in pixels, in (0, CRENDER_WIRE_MAX_WIDTH]
 *   feather    the width of the ramp at each side of a line in pixels, in (0, CRENDER_WIRE_MAX_WIDTH]
 *   opacity    of the lines, in [0, 1]
 *   flags      0
 * CRENDER_EINVAL, before anything is dereferenced or launched, for: a NULL d_winner, P16, line3 or d_color, T < 0,
 * T > 0 without d_tri, H or W < 1, rows outside the frame (y0 < 0, y1 > H, y0 >= y1), a width or feather that is not
 * finite or not in (0, CRENDER_WIRE_MAX_WIDTH], an opacity not in [0, 1], a line3 or fill3 component that is not
 * finite, any flag bit.  T == 0 returns CRENDER_OK without a launch.  One launch; no synchronisation. */
CRENDER_API int crender_wire_overlay(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                     const float *P16, const uint8_t *d_edges, const float *line3, const float *fill3,
                                     float width, float feather, float opacity, float *d_color,
                                     int H, int W, int y0, int y1, unsigned flags, void *stream);

/*
 * The outline: the overlay's lines at FULL width.  A pixel also sees the edges of the triangles that won its
 * neighbours, so the outer half of a silhouette, a border or an occlusion boundary is drawn — on the farther surface
 * or on the background, with the same ramp as inside — and a line is not cut where the triangle that carries it ends.
 * A neighbourhood pass over the winner plane, as crender_ao_shade is; it needs the z plane of the same frame.
 *
 * Result contract.  For every pixel p = (x, y) with y0 <= y < y1:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square root (no
 *                contraction into fused multiply-adds, no reciprocal, denormals kept).
 *   Winners      the winner of a pixel q is VALID if t = d_winner[q] has 0 <= t < T and, with a d_pos_of,
 *                d_pos_of[t] < T.  p is COVERED if its own winner is valid, else it is background.  Nothing is ever
 *                read out of bounds, whatever the planes hold.
 *   Candidates   the valid winners of the pixels q with |qx - x| <= radius_px and |qy - y| <= radius_px that lie on
 *                the frame and in rows y0 <= qy < y1: a strip does not see across its edge.  p itself is among them.
 *   Corners      of candidate t: d_tri[t], or d_tri[d_pos_of[t]] with a d_pos_of, projected as crender_project
 *                projects them: (x_k, y_k, z_k), k = 0, 1, 2 — x and y in pixels, z the projected depth.
 *   Edge mask    the overlay's: bits = d_edges[t] in the caller's order, or 7 without d_edges; bit e draws the edge
 *                from corner e to corner (e + 1) % 3.
 *   Per edge     fx = (float)x, fy = (float)y; for a candidate t and a drawn edge e, a = corner e, b = corner (e + 1) % 3:
 *                  ex = xb - xa,   ey = yb - ya,   px = fx - xa,   py = fy - ya
 *                  s  = (px * ex + py * ey) / (ex * ex + ey * ey)
 *                  s  = s < 0 ? 0 : s;   s = s > 1 ? 1 : s        (selects: a NaN passes both)
 *                  qx = xa + s * ex,   qy = ya + s * ey           (the closest point of the SEGMENT)
 *                  cx = fx - qx,   cy = fy - qy
 *                  d  = sqrtf(cx * cx + cy * cy)
 *                  ze = za + s * (zb - za)                        (projected z is affine on the screen: the edge's
 *                                                                  depth at the closest point)
 *   Hidden lines (t, e) COUNTS at p if t is p's own winner (the same index), or p is background, or
 *                (ze - depth_bias) < d_z[p].  A line behind the surface p shows is never drawn; a silhouette in front
 *                of a farther surface draws its outer half on it.  (False for a NaN: such an edge does not count.)
 *   Minimum      m = +inf; for every (t, e) that counts: if (d < m) m = d.  A NaN (an edge of no length, a corner
 *                that is not finite) is never taken.  A minimum is exact and does not depend on the order: the result
 *                is a function of the SET of candidates.  The kernel visits the taps in an order of its own and skips
 *                a tap whose winner it has just handled.
 *   Window       crender_wire_overlay's statements, unchanged: hi, a, on, the clamp and the opacity.
 *   Colour       a covered pixel: base = fill3 if given, else its own colour; if on, colour_j = base_j * k + line3_j * a
 *                with k = 1.0f - a; if not on, it is stored with fill3 if given and otherwise not written.
 *                A BACKGROUND pixel: base is always its own colour, and it is written only if it is on.
 *                With finite colours no NaN reaches a pixel that is written.
 *   Other planes z, normals and the winner plane are only read.  The colour is read and written at p alone.
 *
 * Limits.  An edge is seen only through pixels its triangle WON within radius_px of p: a sliver that won nothing
 * nearby draws nothing there, as in the overlay, and a line wider than radius_px allows is cut.  For the whole ramp of
 * a line radius_px >= ceil((width + feather) / 2) + 1: the extra pixel is for the won pixel nearest to the closest
 * point.  radius_px = 0 sees the own winner alone (segments instead of the overlay's lines).
 */
#define CRENDER_WIRE_OUTLINE_MAX_RADIUS 8

/* Outline the colour plane d_color float32 [H][W][3] over rows y0 <= y < y1.  crender_wire_overlay's arguments, and
 *   d_z        float32 [H][W]: the z plane of the frame that left d_winner (projected depth, smaller = nearer)
 *   depth_bias finite; in the units of d_z (projected z)
 *   radius_px  0 .. CRENDER_WIRE_OUTLINE_MAX_RADIUS: how far, in pixels, a pixel looks for candidates
 *   flags      0
 * CRENDER_EINVAL, before anything is dereferenced or launched, for every cause of crender_wire_overlay's, a NULL d_z,
 * a depth_bias that is not finite, a radius_px outside 0 .. CRENDER_WIRE_OUTLINE_MAX_RADIUS, any flag bit.  T == 0
 * returns CRENDER_OK without a launch.  One launch with (32 + 2 radius_px)^2 + 32 + 2 radius_px words of LDS; no
 * synchronisation. */
CRENDER_API int crender_wire_outline(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                     const uint32_t *d_pos_of, const float *P16, const uint8_t *d_edges,
                                     const float *line3, const float *fill3, float width, float feather, float opacity,
                                     float depth_bias, int radius_px, float *d_color,
                                     int H, int W, int y0, int y1, unsigned flags, void *stream);

/*
 * Geometric edge anti-aliasing: the coverage of a boundary pixel, computed from the winner plane.  Where a pixel and
 * its left, right, upper or lower neighbour name different triangles, an edge of the nearer of the two crosses the line
 * between the two pixel centres; the rasterizer's own barycentrics at the two centres say where, and so how much of the
 * pixel's cell lies beyond the edge.  The pixel is blended with the ONE neighbour that reaches farthest into its cell.
 * A neighbourhood pass over the winner plane, as crender_wire_outline is; it needs the z plane of the same frame, reads
 * the colour plane and writes a second one.
 *
 * Result contract.  For every pixel p = (x, y) with y0 <= y < y1:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division (no contraction into fused
 *                multiply-adds, no reciprocal, denormals kept).
 *   Winners      v(q), the VALIDATED winner of a pixel q, is crender_wire_outline's: t = d_winner[q] if 0 <= t < T and,
 *                with a d_pos_of, d_pos_of[t] < T; else -1.  Nothing is ever read out of bounds, whatever the planes hold.
 *   Directions   a = 0; for (dx, dy) = (-1, 0), (+1, 0), (0, -1), (0, +1), in this order, with q = (x + dx, y + dy):
 *                  - q off the frame or outside rows y0 <= qy < y1 is passed over: a strip does not see across its edge;
 *                  - wp = v(p), wq = v(q); wp == wq is passed over;
 *                  - near_is_q = wq >= 0 and (wp < 0 or d_z[q] < d_z[p])   (smaller z is nearer; false for a NaN: p is
 *                    then the near one, as it is at equal depths);
 *                  - (n, f, w) = (q, p, wq) if near_is_q, else (p, q, wp): the near pixel, the far one, the near winner.
 *   Corners      of triangle w: d_tri[w], or d_tri[d_pos_of[w]] with a d_pos_of, projected as crender_project projects
 *                them (.pyx:116-130): (x_k, y_k), k = 0, 1, 2.
 *   Barycentrics (bn1, bn2, bn3) at the integer pixel n and (bf1, bf2, bf3) at f: math_utils.pyx:8-34, in its operations
 *                and their order (l01 = x1 - x2, l02 = y1 - y2, l03 = l01 * (y0 - y2) - l02 * (x0 - x2),
 *                b1 = (l01 * (fy - y2) - l02 * (fx - x2)) / l03, and b2, b3 alike: the rasterizer's own).
 *   Exit         t = +inf, k* = none; for k = 1, 2, 3 in order, if bf_k < 0:
 *                  tk = bn_k / (bn_k - bf_k);   if (tk < t) t = tk, k* = k          (a NaN is never taken)
 *                t is where the segment from the near centre to the far one leaves the near triangle: the smallest exit
 *                over the three edge lines, which for a convex triangle is the exit.  Without a k* the far pixel lies
 *                inside the near triangle, no edge lies between the two, and the direction is passed over.
 *   Edge mask    e = k* % 3: b1 vanishes on edge 1 (corner 1 -> 2), b2 on edge 2, b3 on edge 0, in the overlay's
 *                numbering.  With a d_edges the direction is passed over if bit e of d_edges[w] is clear (indexed by w
 *                itself, the caller's order, whatever d_pos_of says).
 *   Share        s = near_is_q ? t - 0.5f : 0.5f - t      (how much of p's cell lies on q's side of the edge)
 *                s = s > 0.5f ? 0.5f : s
 *                if (s > a) a = s, q* = q                  (the first direction wins a tie; a NaN is never taken)
 *   Colour       a == 0: d_out[p] = d_color[p], the bits copied.  Otherwise k = 1.0f - a and, per channel j,
 *                  d_out[p]_j = d_color[p]_j * k + d_color[q*]_j * a
 *   Other planes z, winners, colours and triangles are only read.  Rows outside y0 <= y < y1 of d_out are not touched.
 *
 * The near triangle is taken by depth: the one edge that bounds what is visible decides, from both sides.  Only the
 * single direction with the largest share is blended.  Not covered: the lines where triangles interpenetrate (no edge
 * lies there), neighbours on diagonals, and triangles so small that they won no pixel.
 */

/* Anti-alias rows y0 <= y < y1 of d_color float32 [H][W][3] into d_out float32 [H][W][3].
 *   d_winner, d_z, d_tri, T, d_pos_of, P16, d_edges   as crender_wire_outline takes them
 *   d_out      the result; another plane than d_color (a pixel reads its neighbours' colours)
 *   d_color    only read
 *   flags      0
 * CRENDER_EINVAL, before anything is dereferenced or launched, for: a NULL d_winner, d_z, P16, d_out or d_color, T < 0,
 * T > 0 without d_tri, H or W < 1, rows outside the frame (y0 < 0, y1 > H, y0 >= y1), any flag bit, d_out == d_color.
 * T == 0 makes every winner invalid: the rows are copied.  One launch with 34^2 words of LDS; no synchronisation. */
CRENDER_API int crender_wire_edge_aa(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                     const uint32_t *d_pos_of, const float *P16, const uint8_t *d_edges, float *d_out,
                                     const float *d_color, int H, int W, int y0, int y1, unsigned flags, void *stream);

/*
 * The contour edges: the edge mask of ONE view, for crender_wire_overlay / crender_wire_outline to draw.  A contour
 * edge lies between a triangle that faces the camera and one that faces away; it bounds a smooth body, moves with every
 * pose, and is not among the creases and borders a mask made once per model holds.  The mesh's connectivity does not
 * move: it comes in as the partner table, made once per model (wireframe.edge_partners).
 *
 * The partner table, int32 [T][3] in the caller's triangle order.  Two half-edges are the same edge when their end points
 * have the same float32 bit patterns, as an unordered pair.  Entry [t][e], for the half-edge from corner e to corner
 * (e + 1) % 3 of triangle t:
 *   -1          the edge has no other half-edge (a border);
 *   -2          it has more than one other half-edge;
 *   2 * p + s   otherwise: p is the triangle that holds the other half-edge (t itself for a triangle with two equal
 *               corners), s = 0 if the two half-edges run in opposite directions between the two bit patterns (a
 *               consistent winding), s = 1 if they run the same way.
 * Direction.  A corner is the triple of its coordinates' bit patterns as unsigned integers; triples are compared
 * lexicographically, coordinate 0 first.  A half-edge is SWAPPED if its first corner compares greater than its second,
 * and unswapped otherwise (so also when the two are equal).  Two half-edges of one edge run the same way iff both are
 * swapped or neither is.
 *
 * Result contract.
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division (no contraction into fused
 *                multiply-adds, no reciprocal, denormals kept).
 *   Phase 1      for every triangle t, in the caller's order: q = d_pos_of ? d_pos_of[t] : t.  If q >= T, facing[t] = 0.
 *                Otherwise the corners of d_tri[q] are projected as crender_project projects them (.pyx:116-130), with
 *                xs = (float)(W / 2.0) and ys = (float)(H / 2.0): (x_k, y_k), k = 0, 1, 2.  Nothing is clipped: a corner
 *                behind the camera projects as the rasterizer projects it.  Then
 *                  l1 = x1 - x2,   l2 = y1 - y2
 *                  A  = l1 * (y0 - y2) - l2 * (x0 - x2)       (the denominator l03 of the barycentric b1,
 *                                                              math_utils.pyx:8-34, in its operations and their order)
 *                  facing[t] = A > 0 ? 1 : (A < 0 ? -1 : 0)
 *                A triangle without projected area and every NaN give 0.
 *   Phase 2      for every triangle t, bit e (e = 0, 1, 2) of d_edges[t] is set iff one of these holds, with
 *                v = d_partners[t][e]:
 *                  - d_static is given and bit e of d_static[t] is set (its bits 3 to 7 are ignored);
 *                  - flags has CRENDER_WIRE_CONTOUR_BORDERS, and v is -1 or -2;
 *                  - v >= 0, p = v >> 1 is below T, and facing[t] * facing[p] is -1 for s = v & 1 = 0, or +1 for s = 1.
 *                    A facing of 0 at either side never makes a contour.
 *                Every other v (below -2, or with p >= T) is "no partner": it sets nothing and is never used as an
 *                index, so no table makes the pass read outside d_facing.  Bits 3 to 7 of d_edges[t] are written 0.
 *   Symmetry     a triangle's sign is computed once and both sides of an edge read the same two bytes: if the table
 *                names the two half-edges of an edge as each other's partners, with one s, both get their bit or neither.
 *
 * d_edges is in the caller's order whatever d_pos_of says, as the passes want it.
 */
#define CRENDER_WIRE_CONTOUR_BORDERS 1u     /* also draw the edges without a partner, or with more than one */

/* Classify the edges of T triangles for the view P16 of an H x W frame.
 *   d_tri      float32 [T][3][3], UNPROJECTED camera-frame vertices (may be NULL if T == 0): the last frame's
 *   d_pos_of   NULL, or uint32 [T]: triangle t sits at d_tri[d_pos_of[t]]; an entry >= T gives t the facing 0
 *   P16        HOST float[16], the camera's projection matrix (crender_projection_matrix)
 *   d_partners int32 [T][3], the partner table, in the CALLER's triangle order
 *   d_static   NULL, or uint8 [T] in the caller's order: edges drawn in every view (creases, an explicit mask)
 *   d_facing   int8 [T] of scratch, the caller's: holds the signs of phase 1 afterwards.  Nothing is allocated here.
 *   d_edges    uint8 [T], the result
 *   flags      0 or CRENDER_WIRE_CONTOUR_BORDERS
 * CRENDER_EINVAL, before anything is dereferenced or launched, for: a NULL P16, d_partners, d_facing or d_edges, T < 0,
 * T > 0 without d_tri, H or W < 1, any other flag bit.  T == 0 returns CRENDER_OK without a launch.  Two launches on
 * `stream`, in order; no synchronisation. */
CRENDER_API int crender_wire_contours(const float *d_tri, int64_t T, const uint32_t *d_pos_of, const float *P16,
                                      const int32_t *d_partners, const uint8_t *d_static, int8_t *d_facing,
                                      uint8_t *d_edges, int H, int W, unsigned flags, void *stream);

/*
 * The hidden lines: the edges BEHIND the surface, dashed, as a technical drawing shows the far side of a body.  The
 * overlay, the outline and the contours see an edge only through pixels its own triangle won; a hidden edge belongs to
 * triangles that won nothing where it runs, so no pass over the pixels of the winner plane can draw it.  This one walks
 * the EDGES, with crender_wire_draw's Bresenham, and compares each step's depth with the z plane of the frame.
 *
 * Result contract.
 *
 *   Arithmetic   every float step below is ONE float32 operation, rounded once, with IEEE division (no contraction into
 *                fused multiply-adds, no reciprocal, denormals kept); every integer step is exact.
 *   Key plane    d_key, uint32 [H][W] (crender_wire_key_bytes), is ZERO on entry, and the call leaves it zero.
 *   Segments     segment s = 3 i + e, 0 <= s < 3 T, is the half-edge of triangle i (the caller's order) from corner e to
 *                corner (e + 1) % 3.  It is walked only if bit e of d_edges[i] is set (indexed by i itself, whatever
 *                d_pos_of says; without d_edges all three are; bits 3 to 7 are ignored).  The triangle sits at d_tri[q],
 *                q = d_pos_of ? d_pos_of[i] : i; q >= T skips the segment.  Nothing is ever read out of bounds.
 *   Projection   the corners of d_tri[q] are projected as crender_project projects them (.pyx:116-130), the rasterizer's
 *                own projection: (x_k, y_k, z_k), z_k the projected depth, the unit of d_z.  With a = corner e and
 *                b = corner (e + 1) % 3 the segment is skipped unless both UNPROJECTED z are > 0 (a NaN fails), and
 *                unless fabsf(c) < 2^30 for c = xa, ya, xb, yb (a NaN or an infinity fails): crender_wire_draw's domain.
 *   End points   Xa = (int)rintf(xa), Ya = (int)rintf(ya), and b alike: the nearest pixel centre, ties to even (the
 *                rasterizer samples at integer coordinates).  If (Yb, Xb) is lexicographically smaller than (Ya, Xa),
 *                a and b change places, z_a and z_b with them: the two half-edges of an edge walk the same pixels with
 *                the same operands.  Equal integer end points keep the half-edge's own order; it is one pixel.
 *   Pixels       those of crender_wire_draw's line from (Xa, Ya) to (Xb, Yb) (above: major length el, minor length es,
 *                step t = 0 .. el at the major coordinate advanced by t and the minor by k(t)), without the pixels
 *                off the frame and without those outside rows y0 <= y < y1.
 *   Depth        at step t:  lam = (float)t / (float)el   (0.0f for el = 0)
 *                            dz  = z_b - z_a               (once per segment)
 *                            ze  = z_a + dz * lam
 *                Projected z is affine on the screen: ze is the edge's depth at that step in d_z's units.
 *   Hidden       hidden = d_z[y][x] < (ze - depth_bias).  False for every NaN; the background's 1e6 never hides.  With
 *                CRENDER_WIRE_HIDDEN_USE_WINNER a step with d_winner[y][x] == i, the segment's own triangle, is
 *                visible whatever the depths say.
 *   Stipple      a hidden step is DRAWN iff c % (dash_on + dash_off) < dash_on, c the pixel's coordinate along the
 *                segment's major axis (x if |Xb - Xa| > |Yb - Ya|, else y; never negative on the frame).  The pattern
 *                is anchored to the screen: it continues across chains of short edges and does not depend on the
 *                walking direction.  dash_off = 0 draws a solid line.
 *   Combination  a visible step marks its pixel 2, a drawn hidden step 1, a pixel keeps the largest mark (atomicMax on
 *                d_key).  A pixel is a HIDDEN-LINE pixel iff its mark ends at 1: a hidden edge runs through it and no
 *                walked edge is visible there.  A second launch walks the same steps; the one walker whose
 *                atomicExch(key, 0) returns 1 stores, per channel j,
 *                            k = 1.0f - opacity,   colour_j = colour_j * k + line3_j * opacity
 *                Every other pixel keeps its bits, and the key plane is zero again.  The result is a function of the
 *                SET of marked pixels, not of the order of the walkers.
 *   Other planes z, normals and the winner plane are only read.
 *
 * One pixel wide, not anti-aliased; the dash phase is by screen coordinate, not by arc length.  The winner rule knows
 * the segment's own triangle only: where the partner across the edge won the pixel, the depths decide (depth_bias).
 */
#define CRENDER_WIRE_HIDDEN_USE_WINNER 1u
#define CRENDER_WIRE_MAX_DASH 64

/* Draw the hidden lines of T triangles into d_color float32 [H][W][3] over rows y0 <= y < y1.
 *   d_winner, d_z, d_tri, T, d_pos_of, P16, d_edges   as crender_wire_outline takes them
 *   line3      HOST float[3], the colour of the lines
 *   opacity    of the lines, in [0, 1]
 *   dash_on    pixels drawn per period, 1 .. CRENDER_WIRE_MAX_DASH
 *   dash_off   pixels left out per period, 0 .. CRENDER_WIRE_MAX_DASH
 *   depth_bias finite; in the units of d_z (projected z)
 *   d_key      uint32 [H][W] of crender_wire_key_bytes, zero on entry and zero afterwards
 *   flags      0 or CRENDER_WIRE_HIDDEN_USE_WINNER
 * CRENDER_EINVAL, before anything is dereferenced or launched, checked in THIS order: a NULL d_winner, d_z, P16, line3,
 * d_key or d_color; T < 0; T > 0 without d_tri; H or W < 1; rows outside the frame (y0 < 0, y1 > H, y0 >= y1); H or W
 * above 2^20 (crender_wire_key_bytes' bound); an opacity not in [0, 1]; a line3 component that is not finite; dash_on
 * outside 1 .. CRENDER_WIRE_MAX_DASH or dash_off outside 0 .. CRENDER_WIRE_MAX_DASH; a depth_bias that is not finite;
 * any other flag bit; 3 T beyond what a grid of workgroups of 256 segments can count (T > (2^31 - 1) * 256 / 3).
 * T == 0 returns CRENDER_OK without a launch.  Two launches on `stream`, in order, with 9.2 KB of static LDS each; no
 * synchronisation. */
CRENDER_API int crender_wire_hidden(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                    const uint32_t *d_pos_of, const float *P16, const uint8_t *d_edges, const float *line3,
                                    float opacity, int dash_on, int dash_off, float depth_bias, uint32_t *d_key,
                                    float *d_color, int H, int W, int y0, int y1, unsigned flags, void *stream);

/*
 * The drawing as vectors: crender_wire_hidden's classification of every step, kept.  A hidden-line drawing is a vector
 * object — visible edges solid, hidden edges dashed, at any print size — and the raster pass throws what it knows away
 * into pixels.  These two entries turn the steps of every walked half-edge into maximal RUNS of one class and hand them
 * back as sub-segments of the projected edges, compacted on the device in an order that is a function of the inputs alone.
 *
 * Result contract.
 *
 *   Arithmetic   every float step below is ONE float32 operation, rounded once, with IEEE division (no contraction into
 *                fused multiply-adds, no reciprocal, denormals kept); every integer step is exact.
 *   Segments     crender_wire_hidden's, unchanged: segment s = 3 i + e, i in the caller's order; walked iff bit e of
 *                d_edges[i] is set (all three without d_edges) and q = d_pos_of ? d_pos_of[i] : i is below T; the ends a,
 *                b projected as crender_project projects them; skipped unless both unprojected z are > 0 and
 *                fabsf(c) < 2^30 for c = xa, ya, xb, yb; the ends rounded with rintf; walked from the end whose rounded
 *                (y, x) is smaller (a and b change places, with their depths AND their unrounded coordinates); the
 *                pixels of crender_wire_draw's line, step t = 0 .. el.
 *   Class        of step t: 0 if its pixel is off the frame or outside rows y0 <= y < y1.  Otherwise
 *                  lam = (float)t / (float)el   (0.0f for el = 0),   ze = z_a + (z_b - z_a) * lam
 *                  hidden = d_z[y][x] < (ze - depth_bias)            (false for every NaN)
 *                With CRENDER_WIRE_RUNS_USE_WINNER hidden is cancelled if d_winner[y][x] == i, and, with a d_partners,
 *                also if v = d_partners[i][e] is >= 0 and d_winner[y][x] == v >> 1: a vector drawing draws a mesh edge
 *                ONCE, the edge belongs to two triangles, and either of them winning the pixel means "visible".
 *                Without the flag d_partners is not read.  The class is 1 (HIDDEN) if hidden, else 2 (VISIBLE).
 *   Runs         a run is a maximal interval [t0, t1] of consecutive steps of one segment with the same non-zero class.
 *                A run ends where the walk leaves the frame or the rows: the drawing is clipped to them.  The runs of a
 *                call are ordered by (s, t0), ascending; run k is row k of both results.
 *   d_runs       int32 [N][4]: (s, t0, t1, class).
 *   d_ends       float32 [N][4]: (x0, y0, x1, y1), on the line through the UNROUNDED projected ends A, B in walking order:
 *                  el == 0:   u0 = 0.0f,   u1 = 1.0f
 *                  otherwise  u0 = fmaxf((float)t0 - 0.5f, 0.0f) / (float)el
 *                             u1 = fminf((float)t1 + 0.5f, (float)el) / (float)el
 *                  x(u) = xa * (1.0f - u) + xb * u,   y(u) = ya * (1.0f - u) + yb * u      (left to right)
 *                A run reaches half a step beyond its first and last pixel, but never beyond A or B.  The form gives A
 *                and B back bit for bit at u = 0 and u = 1: chains of fully visible edges close exactly.
 *   Groups       the segments are counted in groups of CRENDER_WIRE_RUNS_GROUP: group g holds segments 256 g .. 256 g + 255.
 *                crender_wire_runs_count writes the number of runs of every group; the caller turns them into the
 *                exclusive prefix d_offsets (int64) and their sum N, allocates, and calls crender_wire_runs_emit with the
 *                SAME operands: run r of group g goes to row d_offsets[g] + r.  Emit stores a row only if its index is
 *                >= 0, below N and below d_offsets[g + 1] (N for the last group): offsets or an N that do not belong to
 *                the operands lose runs, they never make the call write outside d_runs and d_ends.
 *   Other planes everything but d_counts, d_runs and d_ends is only read.
 *
 * Not covered: chaining the runs into polylines, bridging runs of one step.
 */
#define CRENDER_WIRE_RUNS_GROUP 256          /* segments per count */
#define CRENDER_WIRE_RUNS_USE_WINNER 1u

/* The groups of T triangles: ceil(3 T / CRENDER_WIRE_RUNS_GROUP); -1 for T < 0 or 3 T beyond an int32. */
CRENDER_API int64_t crender_wire_runs_groups(int64_t T);

/* Count the runs of every group over rows y0 <= y < y1.
 *   d_winner, d_z, d_tri, T, d_pos_of, P16, d_edges   as crender_wire_hidden takes them
 *   d_partners NULL, or int32 [T][3], the partner table of crender_wire_contours, in the CALLER's triangle order
 *   depth_bias finite; in the units of d_z (projected z)
 *   d_counts   uint32 [crender_wire_runs_groups(T)]: every element is written
 *   flags      0 or CRENDER_WIRE_RUNS_USE_WINNER
 * CRENDER_EINVAL, before anything is dereferenced or launched, checked in THIS order: a NULL d_winner, d_z, P16 or
 * d_counts; T < 0; T > 0 without d_tri; H or W < 1; rows outside the frame (y0 < 0, y1 > H, y0 >= y1); H or W above 2^20
 * (a group's count is a uint32); a depth_bias that is not finite; any other flag bit; 3 T beyond an int32
 * (T > (2^31 - 1) / 3).  T == 0 returns CRENDER_OK without a launch.  One launch on `stream` with 11.3 KB of static LDS;
 * no synchronisation, no atomics. */
CRENDER_API int crender_wire_runs_count(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                        const uint32_t *d_pos_of, const float *P16, const uint8_t *d_edges,
                                        const int32_t *d_partners, float depth_bias, uint32_t *d_counts, int H, int W,
                                        int y0, int y1, unsigned flags, void *stream);

/* Store the runs.  crender_wire_runs_count's operands, unchanged, and
 *   d_offsets  int64 [crender_wire_runs_groups(T)]: the exclusive prefix of the counts
 *   N          the sum of the counts: the rows of d_runs and d_ends
 *   d_runs     int32 [N][4]
 *   d_ends     float32 [N][4]
 * CRENDER_EINVAL, before anything is dereferenced or launched, checked in THIS order: a NULL d_winner, d_z, P16,
 * d_offsets, d_runs or d_ends; then crender_wire_runs_count's checks, with N < 0 between the flag bits and 3 T beyond an
 * int32.  T == 0 and N == 0 return CRENDER_OK without a launch.  One launch on `stream` with 15.4 KB of static LDS; no
 * synchronisation, no atomics. */
CRENDER_API int crender_wire_runs_emit(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                       const uint32_t *d_pos_of, const float *P16, const uint8_t *d_edges,
                                       const int32_t *d_partners, float depth_bias, const int64_t *d_offsets, int64_t N,
                                       int32_t *d_runs, float *d_ends, int H, int W, int y0, int y1, unsigned flags,
                                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_WIRE_H */
