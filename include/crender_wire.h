/*
 * crender_wire.h — C ABI of the wireframe filler (EdgeOnlyPixelBufferFiller) of
 * libcrender_hip.so.  Same conventions as crender_hip.h: raw device pointers, an int
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

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_WIRE_H */
