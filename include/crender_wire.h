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

/*
 * ---- Normal mapping -------------------------------------------------------------------------------------------------
 * Surface detail below the size of a triangle: a deferred pass that PERTURBS THE NORMAL PLANE of the frame a raster
 * launch left, once and right after the draw.  Everything that lights a pixel afterwards reads that plane —
 * crender_guro_illumination, the fused light of crender_tex_shade / crender_mip_shade / crender_aniso_shade and of
 * crender_ssaa_resolve, crender_phong_shade, crender_ao_shade — and so shows the bumps without a change of its own.
 * The two entries live in this unit beside the other passes over the winner plane (crender_wire_edge_aa); "tex.h" and
 * "mip.h" below are include/crender_tex.h and include/crender_mip.h, whose statements are used word for word.
 *
 * A normal map is uint8 [mh][mw][3] in TANGENT SPACE: byte_i = 128 + 127 v_i of a unit vector v = (along u, along v, out
 * of the surface); (128, 128, 255) is "no bump".  Row 0 is the TOP of the image, v = 1, as for a texture.
 *
 * crender_nmap_from_height makes one from a height map, uint8 [mh][mw].  For the texel at (row r, column c), every line
 * ONE float32 operation per operator, rounded once, with IEEE division and square root, no contraction:
 *     k  = scale / 255.0f                                   (once, on the host, in float32)
 *     gx = (float)(h[r][c+1] - h[r][c-1]) * k               (the integer difference, then one conversion)
 *     gy = (float)(h[r-1][c] - h[r+1][c]) * k               (v points up: the row ABOVE minus the row below)
 *     ln = sqrtf((gx*gx + gy*gy) + 1.0f)
 *     vx = -gx / ln,   vy = -gy / ln,   vz = 1.0f / ln
 *     b_i = rintf(v_i * 127.0f + 128.0f)                    (ties to even)
 *     byte_i = !(b_i > 0) ? 0 : (b_i > 255 ? 255 : b_i)     (the clip to 0 .. 255; a NaN, which only an overflowing
 *                                                            scale makes, gives 0)
 * The four neighbours are clamped to the edge (c-1 -> max(c-1, 0), ...), so a 1 x 1 map gives the flat texel; with
 * CRENDER_NMAP_WRAP they wrap around (c-1 -> mw-1 at c = 0, ...).  A flat neighbourhood gives (128, 128, 255).
 */
#define CRENDER_NMAP_WRAP 1u                 /* flag of crender_nmap_from_height: a tiling height map */

/* Fill d_map uint8 [mh][mw][3] from d_height uint8 [mh][mw] (another buffer).
 * CRENDER_EINVAL, before anything is dereferenced or launched, checked in THIS order: a NULL d_height or d_map; mh or mw
 * outside 1 .. 65535; a scale that is not finite; any flag bit but CRENDER_NMAP_WRAP.  One launch; no synchronisation. */
CRENDER_API int crender_nmap_from_height(const uint8_t *d_height, int mh, int mw, float scale, unsigned flags,
                                         uint8_t *d_map, void *stream);

/*
 * Result contract of crender_nmap_shade.  For every pixel (x, y) with y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square root (no
 *                contraction into fused multiply-adds, no reciprocal, denormals kept).  A dot product a.b is
 *                (a0*b0 + a1*b1) + a2*b2 and a length |a| is sqrtf(a.a).
 *   Background   t < 0, t >= T, or d_pos_of[t] >= T: the pixel is not written.  Nothing is ever read out of bounds,
 *                whatever the winner plane holds.
 *   Corners      A, B, C: the three UNPROJECTED vertices of triangle t (d_tri[t], or d_tri[d_pos_of[t]] with a d_pos_of);
 *                (u_k, v_k), k = 0, 1, 2: d_uv[t], indexed by t itself, the caller's order, as in tex.h.
 *   Position     (u, v) at the integer pixel (x, y): Barycentrics, then Affine or (CRENDER_NMAP_PERSPECTIVE) Perspective,
 *                exactly as in tex.h.
 *   Sample       s, float32 [3], of the map at (u, v):
 *                  no filter flag           the texel rule of tex.h (nearest);
 *                  CRENDER_NMAP_BILINEAR    the Bilinear statement of tex.h;
 *                  CRENDER_NMAP_CHAIN       d_map is the mip chain of the mh x mw map in mip.h's layout (crender_mip_build:
 *                                           L = 1 + floor(log2(max(mh, mw))) levels, h_k = max(1, mh >> k), packed
 *                                           tightly), and the sample is mip.h's trilinear one: Neighbours, Footprint and
 *                                           Level word for word (with (th, tw) = (mh, mw)), then a = Bilinear on level
 *                                           l0 and, where f != 0, b = Bilinear on level l0 + 1 and s = a*(1 - f) + b*f,
 *                                           left to right.  The levels are box averages of the BYTES, not re-normalised.
 *   Decode       m_i = (s_i - 128.0f) / 127.0f;  m_i = m_i < -1 ? -1 : m_i      (byte 0 decodes to -1, as byte 1 does)
 *                mx = m_0 * strength,   my = m_1 * strength,   mz = m_2
 *   Tangents     of the TRIANGLE (the frame is per triangle, not smoothed over the mesh):
 *                  e1 = B - A,   e2 = C - A
 *                  du1 = u1 - u0,  dv1 = v1 - v0,  du2 = u2 - u0,  dv2 = v2 - v0
 *                  det = du1*dv2 - du2*dv1,     sg = det < 0 ? -1 : 1
 *                  Tt_j = (e1_j*dv2 - e2_j*dv1) * sg,     Bt_j = (e2_j*du1 - e1_j*du2) * sg       (j = 0, 1, 2)
 *                Tt points along increasing u on the surface, Bt along increasing v (both up to a positive factor).
 *   Frame        around the pixel's STORED normal n = d_normal[y][x]:
 *                  nl = |n|,   Nu = n / nl
 *                  d  = Nu.Tt,   Tp = Tt - Nu*d,   tl = |Tp|,   Tu = Tp / tl
 *                  Bp = (Nu1*Tu2 - Nu2*Tu1,  Nu2*Tu0 - Nu0*Tu2,  Nu0*Tu1 - Nu1*Tu0)
 *                  if (Bp.Bt < 0) Bp = -Bp
 *                The stored normals may point either way relative to the winding: the handedness comes from the uv.
 *   Result       out_j = (Tu_j*mx + Bp_j*my) + Nu_j*mz.  Not normalised: guro_factor divides by the length.  out.Nu = mz
 *                up to rounding, so a bump never turns a normal past 90 degrees.
 *   Write        d_normal[y][x] = out iff
 *                  (det > 0 || det < 0) && nl > 0 && tl > 0 && (mx < 0 || mx > 0 || my < 0 || my > 0)
 *                Every NaN makes the condition false (the last clause is "mx != 0 || my != 0" for numbers).  A flat
 *                texel, strength = 0, a triangle whose uv are degenerate, a zero, NaN or infinite normal, a tangent
 *                parallel to the normal and a sample that is not a number therefore keep the pixel's bits, and with a
 *                finite strength no NaN is ever written.
 *   Other planes d_normal is read and written at (x, y) alone.  z, colours and the winner plane are not among the
 *                arguments; the winner plane, the triangles, the uv and the map are only read.
 *
 * Not covered: per-vertex (smoothed) tangents — a coarse mesh shows facets in the bumps; anisotropic filtering of the
 * map; re-normalised mip levels or variance-to-roughness (Toksvig); parallax or displacement; object-space maps.
 */
enum {
    CRENDER_NMAP_PERSPECTIVE = 1u,   /* perspective-correct uv (tex.h); default: affine                          */
    CRENDER_NMAP_BILINEAR = 2u,      /* four texels (tex.h); default: the nearest one                            */
    CRENDER_NMAP_CHAIN = 4u          /* d_map is a mip chain, the filter is trilinear; not with CRENDER_NMAP_BILINEAR */
};

/* Perturb rows y0 <= y < y1 of the normal plane d_normal float32 [H][W][3].
 *   d_winner, d_tri, T, d_pos_of, P16   as crender_wire_overlay takes them
 *   d_uv       float32 [T][3][2], (u, v) per corner in the CALLER's triangle order (may be NULL if T == 0)
 *   d_map      uint8 [mh][mw][3], or with CRENDER_NMAP_CHAIN the chain of crender_mip_build(map, mh, mw)
 *   mh, mw     the map's size (level 0's), 1 .. 65535
 *   strength   finite; scales the two tangent components of the decoded vector (0: nothing is written)
 * CRENDER_EINVAL, before anything is dereferenced or launched, checked in THIS order: a NULL d_winner, P16, d_map or
 * d_normal; T < 0; T > 0 without d_tri or without d_uv; H or W < 1; rows outside the frame (y0 < 0, y1 > H, y0 >= y1);
 * mh or mw outside 1 .. 65535; a strength that is not finite; an unknown flag bit; CRENDER_NMAP_CHAIN together with
 * CRENDER_NMAP_BILINEAR.  T == 0 returns CRENDER_OK without a launch.  One launch (the chain's level offsets travel in its
 * arguments); no synchronisation. */
CRENDER_API int crender_nmap_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                   const float *P16, const float *d_uv, const uint8_t *d_map, int mh, int mw,
                                   float strength, float *d_normal, int H, int W, int y0, int y1, unsigned flags,
                                   void *stream);

/*
 * ---- Environment mapping --------------------------------------------------------------------------------------------
 * What is around the model: a deferred pass that looks a DIRECTION up in a cube map, for the covered pixels the
 * direction in which the surface mirrors the eye (reflections), for the others the pixel's own view ray (a skybox).
 * Everything it needs is resident after a frame: the winner plane and the triangles give the surface point, exactly as
 * crender_phong_shade rebuilds it, the normal plane — perturbed by crender_nmap_shade or not — the normal, the
 * projection a background pixel's ray.  The entry lives in this unit beside the other passes over the winner plane;
 * "tex.h", "phong.h" and "ao.h" below are include/crender_tex.h, crender_phong.h and crender_ao.h, whose statements are
 * used word for word.
 *
 * Result contract of crender_env_shade.  For every pixel (x, y) with 0 <= x < W, y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square root (no
 *                contraction into fused multiply-adds, no reciprocal, denormals kept).  Constants named "host" are
 *                computed in double and rounded once to float.
 *   Frames       the camera's frame is the rasterizer's: x grows with the column, y with the row, z goes into the screen,
 *                the eye is at the origin.  The environment's frame is the camera's turned by M (below).
 *   Environment  a cube map uint8 [6][S][S][3], 1 <= S <= CRENDER_ENV_MAX_SIDE, the faces in the order +x, -x, +y, -y,
 *                +z, -z of the environment's frame.  The +z face is what the camera itself sees (under the identity);
 *                the others are that frame turned by quarter turns.  Row 0 of a face is where tc (below) is smallest.
 *   Face         of a direction d: a = (|d0|, |d1|, |d2|); the major axis is x if a0 >= a1 && a0 >= a2, else y if
 *                a1 >= a2, else z (so a NaN falls through to z); ma is that magnitude, face = 2 axis + (d_axis < 0), and
 *                    face   +x    -x    +y    -y    +z    -z
 *                    sc    -d2    d2    d0    d0    d0   -d0
 *                    tc     d1    d1   -d2    d2    d1    d1
 *                d is USABLE when ma > 0 && ma < INFINITY.  A pixel whose direction is not usable is not written.
 *   Sample       e = the Bilinear statement of tex.h, unchanged, on that face taken as an S x S texture, at
 *                    tu = (sc / ma + 1.0f) * 0.5f,     tv = (1.0f - tc / ma) * 0.5f
 *                (the row grows with tc; indices are clamped to the face: nothing is filtered across faces).
 *   Two levels   with d_faces1 (side S1) and 0 < level_frac = f < 1: e_c = e0_c * (1.0f - f) + e1_c * f, both levels
 *                sampled at the same direction.  Which two levels of a chain they are is the host's matter.
 *   Orientation  M9 is a row-major 3 x 3: d_i = (M[i][0]*r0 + M[i][1]*r1) + M[i][2]*r2.
 *
 *   CRENDER_ENV_REFLECT, for a COVERED pixel (0 <= t < T and, with a d_pos_of, d_pos_of[t] < T), unless reflectivity == 0
 *   (then no covered pixel is written):
 *     Point      p: project the winner, the rasterizer's barycentrics b_k, then phong.h's "Surface point":
 *                    q_k = b_k / z_k,   s = (q1 + q2) + q3,   p_c = ((A_c*q1 + B_c*q2) + C_c*q3) / s
 *     Mirror     n = d_normal[y][x];  nn = (n0*n0 + n1*n1) + n2*n2,  ni = (n0*p0 + n1*p1) + n2*p2,
 *                    k = (2.0f * ni) / nn,      r_c = p_c - k * n_c
 *                (not normalised: the face and the two quotients do not depend on |r|; and the same for n and -n).
 *                d = M r, e the sample.
 *     Weight     pp = (p0*p0 + p1*p1) + p2*p2,   c = fabsf(ni) / (sqrtf(nn) * sqrtf(pp)),   m = 1.0f - c,
 *                    m = m < 0 ? 0 : m,   m = m > 1 ? 1 : m;   a NaN m makes the pixel NOT written
 *                    m5 = ((m*m) * (m*m)) * m,     w = reflectivity * (f0 + one_minus_f0 * m5)
 *                with host one_minus_f0 = (float)(1.0 - (double)f0): Schlick's weight, f0 facing the eye, 1 at a
 *                grazing angle.
 *     Result     colour_c = colour_c * (1.0f - w) + (e_c * tint_c) * w
 *
 *   CRENDER_ENV_BACKGROUND, for every pixel of the rows that is NOT covered (winners that name no triangle included):
 *     Ray        with ao.h's host constants xs, ys, kx, ky: r = (((float)x - xs) * kx, ((float)y - ys) * ky, 1.0f)
 *                d = M r, e the sample.
 *     Result     colour_c = e_c * background_gain
 *
 *   Other planes z, normals and the winner plane are only read.  Nothing is ever read out of bounds, whatever the
 *                planes hold.
 *
 * Not covered: filtering across the seams of the faces; prefiltered (cosine or GGX) chains — two levels are a blur, not
 * a roughness model —; per-pixel reflectivity; refraction; diffuse irradiance; reflections that see the model itself.
 */
#define CRENDER_ENV_REFLECT 1u               /* covered pixels mirror the environment                                   */
#define CRENDER_ENV_BACKGROUND 2u            /* the other pixels of the rows show it                                    */
#define CRENDER_ENV_MAX_SIDE 8192

/* Shade rows y0 <= y < y1 of the colour plane d_color float32 [H][W][3].
 *   d_winner, d_tri, T, d_pos_of, P16   as crender_wire_overlay takes them; d_tri is read with REFLECT only
 *   d_normal   float32 [H][W][3], the normal plane of the frame; may be NULL without REFLECT
 *   d_faces0   uint8 [6][S0][S0][3]
 *   d_faces1   NULL, or uint8 [6][S1][S1][3]: the second level
 *   level_frac the weight of the second level, 0 < level_frac < 1; 0 without one
 *   M9         HOST float[9], finite: the orientation
 *   reflectivity, f0   0 .. 1
 *   tint3      HOST float[3], finite: a factor per channel of the reflected sample
 *   background_gain    finite, >= 0
 *   flags      CRENDER_ENV_REFLECT, CRENDER_ENV_BACKGROUND or both
 * CRENDER_EINVAL ("crender_env_shade: ..."), before anything is dereferenced or launched, checked in THIS order: a NULL
 * d_winner, P16, d_faces0, M9, tint3 or d_color, or a NULL d_normal with REFLECT; T < 0; T > 0 without d_tri; H or W < 1;
 * rows outside the frame (y0 < 0, y1 > H, y0 >= y1); S0 outside 1 .. 8192 or S1 outside 0 .. 8192; d_faces1, S1 and
 * level_frac that are neither all given (S1 >= 1, 0 < level_frac < 1) nor all absent (NULL, 0, 0); an M9, tint3 or
 * background_gain that is not finite, a reflectivity or f0 outside [0, 1], a negative background_gain; with BACKGROUND a
 * P16 whose entry 0 or 5 is zero or not finite; an unknown flag bit, or neither flag.  With REFLECT alone T == 0 and
 * reflectivity == 0 return CRENDER_OK without a launch; with BACKGROUND T == 0 paints every pixel of the rows.  One
 * launch (M9, tint3 and the coefficients travel in its arguments); no synchronisation. */
CRENDER_API int crender_env_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                  const float *P16, const float *d_normal, const uint8_t *d_faces0, int S0,
                                  const uint8_t *d_faces1, int S1, float level_frac, const float *M9, float reflectivity,
                                  float f0, const float *tint3, float background_gain, float *d_color, int H, int W,
                                  int y0, int y1, unsigned flags, void *stream);

/*
 * ---- Depth of field -------------------------------------------------------------------------------------------------
 * The frame through a lens instead of a pinhole: a post-process that blurs every pixel by its CIRCLE OF CONFUSION, which
 * the z plane gives exactly.  A gather: a pixel sums the colours of the pixels around it, each weighted by how much of its
 * own disc reaches the pixel, so that what is in front spreads over what lies behind it and a blurred background does
 * not bleed over something sharper in front of it.  The colour plane is only read and the result goes to a plane of its
 * own (a pixel reads its neighbours' colours), as crender_wire_edge_aa's.  The entry lives in this unit beside the other
 * passes over the winner plane; "ao.h" below is include/crender_ao.h.
 *
 * Result contract of crender_dof_blur.  For every pixel p = (x, y) with 0 <= x < W and y0 <= y < y1:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square root (no
 *                contraction into fused multiply-adds, no reciprocal, denormals kept).  Rf = (float)max_radius,
 *                pi = (float)3.14159265358979323846 = 0x40490FDB.
 *   Signed circle of confusion s of a pixel q, in pixels; negative in front of the focal plane, positive behind it:
 *     covered    (t = d_winner[q] with 0 <= t < T; d_pos_of is not looked at):  with P10 = P16[10], P14 = P16[14]
 *                    zv = P14 / (z - P10)                         (the view depth, as ao.h rebuilds it)
 *                    d  = zv - focus
 *                    d  = d > band ? d - band : (d < -band ? d + band : 0.0f)     (a NaN d gives 0)
 *                    s  = aperture * (d / zv)
 *     uncovered  s = aperture                                     (the background is at infinity)
 *     clamp      s = s > Rf ? Rf : (s < -Rf ? -Rf : s)            (a NaN stays a NaN)
 *     off the frame or outside the rows:  s = NaN; such a pixel contributes nowhere, and none of its planes is read.
 *                c  = fabsf(s)                                    the blur radius
 *                ia = 1.0f / (1.0f + pi * (s * s))                the reciprocal of the footprint: one division per
 *                                                                 pixel, none per tap
 *   Taps         Sw = S_0 = S_1 = S_2 = +0.  For dy = -max_radius .. max_radius (outer) and dx = -max_radius ..
 *                max_radius (inner), both ascending, q = p + (dx, dy) and dist = sqrtf((float)(dx*dx + dy*dy)):
 *                    q LIES BEHIND p if s_q > s_p                 (s grows with the view depth)
 *                    if q lies behind p and c_p < c_q:  r = c_p, a = ia_p
 *                    otherwise:                         r = c_q, a = ia_q
 *                    k = (r + 1.0f) - dist;   the tap is TAKEN iff k > 0    (every NaN fails)
 *                    w = (k < 1.0f ? k : 1.0f) * a
 *                    Sw = Sw + w;   S_j = S_j + w * d_color[q]_j             (multiply, then add; j = 0, 1, 2)
 *                A tap that is not taken changes nothing, whatever d_color[q] holds.
 *   Result       if no tap other than (0, 0) was taken, or Sw > 0 is false:  d_out[p] = d_color[p], the bits copied
 *                (a -0 and every NaN colour are kept).  Otherwise d_out[p]_j = S_j / Sw.  Where a NaN or an infinite
 *                colour was taken, a sum or the quotient may be a NaN: WHICH NaN (sign, payload) is not stated.
 *   Other planes z, winners and colours are only read; d_tri and d_pos_of are never read.  Rows outside y0 <= y < y1 of
 *                d_out are not touched.  Nothing is ever read out of bounds, whatever the planes hold.
 *
 * Consequences.  aperture == 0 makes every c zero or NaN and the rows are copied bit for bit.  A pixel with c == 0 out
 * of reach of every blurred one (no q with r + 1 > dist) keeps its bits.  On a frame of one colour a blurred pixel
 * differs from that colour by the rounding of the sums and the quotient only.  A tap beyond ceil(the largest c around)
 * is never taken (r + 1 <= ceil + 1 <= dist, both roundings monotone): an implementation may stop there.
 *
 * Not covered: radii above CRENDER_DOF_MAX_RADIUS (the staged tile and its halo, five words a pixel, fill the 64 KB of
 * LDS at 12); what a blurred foreground hides (its colours were never rendered: the gather renormalises over what is
 * there); bokeh shapes (the disc is round and flat, with a one-pixel ramp).
 */
#define CRENDER_DOF_MAX_RADIUS 12

/* Blur rows y0 <= y < y1 of d_color float32 [H][W][3] into d_out float32 [H][W][3].
 *   d_winner   int32 [H][W]; with T it says which pixels are covered
 *   d_z        float32 [H][W], the z plane of the frame
 *   d_tri, d_pos_of   accepted (the passes' common frame) and never read; may be NULL
 *   T          the triangles of the frame: a winner outside [0, T) is background
 *   P16        HOST float[16], crender_projection_matrix's
 *   d_color    only read
 *   focus      the view depth in focus (cython3dmodelrenderer_amd.depth_of_field.view_depth of a z); finite, > 0
 *   band       the half width of the range of view depths around focus that stays sharp; finite, >= 0
 *   aperture   the blur radius in pixels at infinity; finite, >= 0
 *   max_radius 1 .. CRENDER_DOF_MAX_RADIUS: the clamp of every radius, and the reach of the taps
 *   d_out      the result; another plane than d_color
 *   flags      0
 * CRENDER_EINVAL ("crender_dof_blur: ..."), before anything is dereferenced or launched, checked in THIS order: a NULL
 * d_winner, d_z, P16, d_color or d_out; T < 0; H or W < 1; rows outside the frame (y0 < 0, y1 > H, y0 >= y1); any flag
 * bit; d_out == d_color; a P16 that is not of crender_projection_matrix's shape (ao.h's two checks, in its words); a focus
 * that is not finite and > 0; a band, then an aperture, that is not finite and >= 0; max_radius outside 1 .. 12.
 * T == 0 makes every pixel background (s = aperture).  One launch with 5 (32 + 2 max_radius)^2 + 173 words of LDS
 * (62 720 + 692 bytes at 12: below 64 KB, no launch attribute); no synchronisation. */
CRENDER_API int crender_dof_blur(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                 const uint32_t *d_pos_of, const float *P16, const float *d_color, float focus, float band,
                                 float aperture, int max_radius, float *d_out, int H, int W, int y0, int y1, unsigned flags,
                                 void *stream);

/* ---- Transparency: depth peeling by depth key, blended front to back -------------------------------------------------
 *
 * A frame keeps one fragment per pixel, the one with the least 64-bit key fragment_key(z, i) (csrc/raster_math.h: the
 * order-preserving map of z in the high word, 0xFFFFFFFE - i in the low one), and leaves the key's two halves behind:
 * the z plane and the winner plane.  crender_peel_next finds, per pixel, the fragment with the least key STRICTLY ABOVE
 * a given layer's: the next layer behind it.  No epsilon; coplanar duplicates peel one by one, the highest index first.
 * crender_peel_blend puts a layer under what is in front of it.  Every operation below is one IEEE binary32 operation,
 * nothing contracted, in the order written.
 *
 * Fragments.   THE FRAGMENTS OF THE FRAME AT pixel p = (x, y) are the pairs (i, z), i a triangle index in the caller's
 *              order (the winner plane's), for which: triangle i lies in d_tri (under d_pos_of: d_pos_of[i] < T);
 *              backface(n0z, n1z, n2z) of its three normals' z is false (n0z + n1z + n2z >= 0 is the back face); its
 *              pixel_box on the W x H frame is not empty and holds p; with the corners projected as crender_project does,
 *              the three barycentrics b1, b2, b3 at (x, y) (three correctly rounded divisions) are none of them < 0 (a
 *              NaN passes); z = z0*b1 + z1*b2 + z2*b3, left to right, is not NaN; and fragment_key(z, i) is below the
 *              cleared key make_key(zord(1e6f), 0xFFFFFFFF).
 * Next layer.  The given layer is VALID at p if its winner w satisfies 0 <= w < T (and under d_pos_of: d_pos_of[w] < T)
 *              and its z is not NaN.  Then K = fragment_key(z, w), and the result at p names the fragment of the frame
 *              at p with the least key k > K: its index, and ITS z, the value of the sum above (a -0 stays -0; not the
 *              key's word decoded).  If the layer is not valid at p or no fragment has k > K, the result is winner -1
 *              and z 1e6f: what a cleared frame holds, which is not valid again — an exhausted pixel stays exhausted.
 * Blend.       Per pixel p of the rows, with FIRST and LAST the two flags:
 *                  t = FIRST ? 1.0f : d_trans[p]
 *                  if the layer's winner w is a triangle (as above) and t > 0:
 *                      a = d_alpha[w];  a = a > 0 ? a : 0  (a NaN gives 0);  a = a > 1 ? 1 : a
 *                      c = d_front[p] if FIRST and d_front is given; otherwise the colour shade_fragment gives triangle w
 *                          at p: c_j = col0_j*b1 + col1_j*b2 + col2_j*b3, and with light3 times guro_factor of the
 *                          normal interpolated the same way — the bits a frame stores for this fragment
 *                      g = t * a
 *                      d_out[p]_j = FIRST ? g * c_j : d_out[p]_j + g * c_j          (multiply, then add)
 *                      d_trans[p] = t * (1.0f - a)
 *                  otherwise, if FIRST:  d_out[p] = (0, 0, 0), d_trans[p] = 1
 *                  otherwise nothing is written
 *                  with LAST, after that step, where d_trans[p] > 0:  d_out[p]_j = d_out[p]_j + d_trans[p] * background_j
 * Consequences. alpha == 1 everywhere gives the front layer's colours bit for bit (1 * c, a -0 kept) and the background
 *              elsewhere; alpha == 0 everywhere gives the background everywhere a colour is finite; a pixel whose
 *              transmittance has reached 0 is never written again, so a NaN behind an opaque layer does not spread.
 *
 * Not covered: back faces behind a transparent front (the frame's culling applies to every layer); an early exit when a
 * layer comes out empty; per-vertex or textured alpha; refraction.
 */
#define CRENDER_PEEL_FIRST 1u                /* the layer is the front one: d_out and d_trans are written, not read   */
#define CRENDER_PEEL_LAST 2u                 /* the background shows through what transmittance is left               */
#define CRENDER_PEEL_MAX_LAYERS 16           /* what the Python layer peels at most (the entries know no limit)       */

/* The layer behind a layer, rows y0 <= y < y1.
 *   d_winner, d_z   int32 / float32 [H][W]: the given layer (a frame's planes, or an earlier result)
 *   d_tri      float32 [T][3][3], unprojected, in the order d_pos_of describes;  T at most 2^31 - 1
 *   d_pos_of   NULL, or uint32 [T]: where the caller's triangle i lies in d_tri (a value >= T: nowhere)
 *   P16        HOST float[16], crender_projection_matrix's
 *   d_nrm      float32 [T][3][3], in d_tri's order
 *   d_keys     crender_atomic_scratch_bytes(H, W) bytes of scratch, 8-byte aligned; its rows are overwritten
 *   d_winner_out, d_z_out   the result; other planes than the given layer's.  Rows outside are not touched
 *   flags      0
 * CRENDER_EINVAL ("crender_peel_next: ..."), before anything is dereferenced or launched, checked in THIS order: a NULL
 * d_winner, d_z, P16, d_keys, d_winner_out or d_z_out; T < 0; d_tri or d_nrm NULL with T > 0; H or W < 1; rows outside
 * the frame; any flag bit; T > 2^31 - 1; d_winner_out == d_winner or d_z_out == d_z.
 * Three launches (two with T == 0, which makes every pixel of the rows empty); no synchronisation. */
CRENDER_API int crender_peel_next(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                  const uint32_t *d_pos_of, const float *P16, const float *d_nrm, void *d_keys,
                                  int32_t *d_winner_out, float *d_z_out, int H, int W, int y0, int y1, unsigned flags,
                                  void *stream);

/* One layer under what is in front of it, rows y0 <= y < y1.
 *   d_winner   int32 [H][W]: the layer's winner plane
 *   d_tri, d_pos_of, P16   as above
 *   d_col, d_nrm   float32 [T][3][3], in d_tri's order
 *   d_alpha    float32 [T] in the CALLER's order: indexed by the winner word
 *   light3     NULL, or HOST float[3]: the fused Guro light (crender_plan_set_light's vector)
 *   d_front    NULL, or float32 [H][W][3]: the front layer's colours as they are (only with CRENDER_PEEL_FIRST)
 *   background3   HOST float[3], finite
 *   d_trans    float32 [H][W]: the transmittance, written by FIRST, read and written otherwise
 *   d_out      float32 [H][W][3]: the sum, likewise
 * CRENDER_EINVAL ("crender_peel_blend: ..."), before anything is dereferenced or launched, checked in THIS order: a NULL
 * d_winner, P16, background3, d_trans or d_out; T < 0; d_tri, d_col, d_nrm or d_alpha NULL with T > 0; H or W < 1; rows
 * outside the frame; a flag bit other than the two; d_front without CRENDER_PEEL_FIRST; d_out == d_front; a background3,
 * then a light3, that is not finite.  One launch, no LDS; no synchronisation. */
CRENDER_API int crender_peel_blend(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                   const float *P16, const float *d_col, const float *d_nrm, const float *d_alpha,
                                   const float *light3, const float *d_front, const float *background3, float *d_trans,
                                   float *d_out, int H, int W, int y0, int y1, unsigned flags, void *stream);

/*
 * ---- Bloom ----------------------------------------------------------------------------------------------------------
 * Bloom and tone mapping: a glow around what is brighter than a threshold, and a curve that brings the range back into
 * 0 .. 255.  A post-process over ANY float32 image [H][W][3] — the filler's colour plane, or the tensor of
 * crender_wire_edge_aa, crender_dof_blur, crender_peel_blend or crender_ssaa_resolve — and so the first stage that can
 * follow any of them.  The blur is SEPARABLE: the rows into a scratch plane, then the columns.  The entry lives in this
 * unit beside the other neighbourhood passes.
 *
 * Result contract of crender_bloom.  Every step below is ONE float32 operation, rounded once, with IEEE division and
 * square root (no contraction into fused multiply-adds, no reciprocal, denormals kept); no exponential, power or
 * logarithm is taken on the device: the weights w[0 .. radius] come from the host.  With src = d_src, R = radius:
 *
 *   1 Bright     per pixel (r, g, b) of src:  m = r; if (g > m) m = g; if (b > m) m = b;  k = m - threshold.
 *                If k > 0 is false (a NaN m included) bright = (+0, +0, +0).  Otherwise q = k / m and
 *                bright = (r * q, g * q, b * q): the hue is kept, at one division per bright pixel.
 *   2 Rows       hb[y][x][c] = sum over dx = -R .. R, in that order and starting from +0, of w[|dx|] * bright[y][x + dx][c]:
 *                each tap one multiply, then one add.  A column outside 0 .. W - 1 has the bright value +0, and is
 *                still added.
 *   3 Columns    g[y][x][c] = sum over dy = -R .. R of w[|dy|] * hb[y + dy][x][c], in the same manner.  A row outside
 *                y0 .. y1 - 1 has hb = +0: the strip does not see across its edge.
 *   4 Composite  t_c = intensity * g_c.  If all three t are +-0:  v = src[y][x], bit for bit (a -0 and every NaN kept).
 *                Otherwise v_c = src_c + t_c.  (The test is on t, not on g, so that an intensity of 0 keeps a -0 of
 *                the source within a glow's reach: -0 + +0 would be +0.)
 *   5 Tone       only with CRENDER_BLOOM_REINHARD, CRENDER_BLOOM_GAMMA2 or exposure != 1; otherwise o = v.
 *                    a = v * exposure;  a = a > 0 ? a : 0  (a NaN gives 0);  a = a * inv255
 *                    L = a                                             without CRENDER_BLOOM_REINHARD
 *                    L = (a * (1 + a * inv_white2)) / (1 + a)          with it
 *                    L = sqrtf(L)                                      with CRENDER_BLOOM_GAMMA2
 *                    o = L * 255
 *                inv255 = (float)(1.0 / 255.0) = 0x3B808081.  inv_white2 is the caller's (float)(1.0 / (white * white)),
 *                computed in double and rounded once; 0 is the plain operator a / (1 + a).
 *   6 Clamp      o = o > clamp ? clamp : o                             (a NaN stays a NaN; +inf clamps nothing)
 *   7 Store      d_out[Y][x][c] = o as float32, or with CRENDER_BLOOM_U8 crender_present_u8's cast of o (truncation to
 *                int32, INT_MIN for a NaN or out of range, the low byte);  Y = y, or with CRENDER_BLOOM_FLIP H - 1 - y:
 *                both as crender_ssaa_resolve stores them.
 *   Other planes d_src is only read.  Rows y0 .. y1 - 1 of d_scratch hold hb on return; its other rows, and the rows of
 *                d_out that no Y names, are not touched.  Nothing is read out of bounds, whatever the planes hold.
 *
 * Consequences.  intensity == 0 copies the source (every t is +-0 for a finite g), and so does a threshold above every
 * pixel.  A pixel out of reach of every bright pixel keeps its bits.  The weights are finite, so a neighbourhood whose
 * bright or hb values are all +-0 sums to +0 exactly: an implementation may skip it.  An infinite colour under a zero
 * weight gives a NaN; WHICH NaN (sign, payload) a step computes is not stated, copied NaNs keep every bit.
 *
 * Not covered: radii above CRENDER_BLOOM_MAX_RADIUS and mip pyramids, a soft knee, luminance-weighted keys, operators
 * other than Reinhard's, sRGB's 2.4 curve (gamma is 1 or 2), both directions fused into one launch.
 */
#define CRENDER_BLOOM_MAX_RADIUS 32
#define CRENDER_BLOOM_U8 1u                  /* d_out is uint8 [H][W][3]                                                */
#define CRENDER_BLOOM_FLIP 2u                /* rows are stored bottom up                                               */
#define CRENDER_BLOOM_REINHARD 4u            /* rule 5's operator                                                       */
#define CRENDER_BLOOM_GAMMA2 8u              /* rule 5's square root                                                    */

/* Bloom rows y0 <= y < y1 of d_src float32 [H][W][3] into d_out.
 *   d_src      only read
 *   threshold  what the largest channel must exceed to glow; >= 0 (+inf: nothing glows)
 *   weights    HOST float[radius + 1], finite: w[k] weighs the taps at distance k (cython3dmodelrenderer_amd.bloom.gaussian).
 *              Copied into the kernel arguments: the caller's array is free on return.
 *   radius     1 .. CRENDER_BLOOM_MAX_RADIUS
 *   intensity  finite, >= 0
 *   exposure   finite, >= 0
 *   inv_white2 >= 0
 *   clamp      +inf means none; not NaN
 *   d_scratch  float32 [H][W][3], the caller's: hb
 *   d_out      float32 [H][W][3], or uint8 [H][W][3] with CRENDER_BLOOM_U8; aliases neither d_src nor d_scratch
 * CRENDER_EINVAL ("crender_bloom: ..."), before anything on the device is dereferenced or launched, checked in THIS
 * order: H or W < 1; rows outside the frame (y0 < 0, y1 > H, y0 >= y1); a NULL d_src, weights, d_scratch or d_out; a radius
 * outside 1 .. 32; a weight that is not finite; a threshold that is negative or NaN; an intensity, then an exposure, that
 * is not finite and >= 0; an inv_white2 that is negative or NaN; a NaN clamp; a flag bit other than the four; d_out,
 * d_scratch and d_src that are not three planes.  Two launches, each with 3 * 32 * (32 + 2 radius) words of LDS (36 864
 * bytes at 32; the second four words more: below 64 KB, no launch attribute); no synchronisation. */
CRENDER_API int crender_bloom(const float *d_src, float threshold, const float *weights, int radius,
                              float intensity, float exposure, float inv_white2, float clamp,
                              float *d_scratch, void *d_out, int H, int W, int y0, int y1,
                              unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_WIRE_H */
