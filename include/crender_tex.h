/*
 * crender_tex.h — C ABI of the deferred texture pass of libcrender_hip.so: per-pixel texture
 * mapping over the winner plane a raster launch left (crender_render_model with a d_winner).
 * Same conventions as crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this
 * header as it covers crender_wire.h: raw device pointers, an int status (CRENDER_OK or a
 * CRENDER_E* code, text in crender_last_error()), work enqueued on `stream` and nothing
 * synchronised.  ".pyx" is the reference's crender/cy/pixel_buffer_filler/
 * advanced_pixel_buffer_filler.pyx, "model.py" its crender/cy/data_structures/model.py.
 *
 * Result contract.  For every pixel (x, y) with y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division
 *                (no contraction into fused multiply-adds, denormals kept).
 *   Background   t < 0 or t >= T: the colour is left as it is (but see "Fused light").  Nothing is
 *                ever read out of bounds, whatever the winner plane holds.
 *   Barycentrics the three vertices of triangle t — d_tri[t], or d_tri[d_pos_of[t]] with a
 *                d_pos_of — are projected as crender_project projects them (.pyx:116-130), and
 *                (b1, b2, b3) are the barycentrics of the integer pixel (x, y) in the projected
 *                triangle (math_utils.pyx:8-34): the chain the raster resolve evaluates.
 *   Affine       (default) u = u0*b1 + u1*b2 + u2*b3, left to right, and v alike — how the
 *                reference interpolates colours and normals (.pyx:226-231).  (u_k, v_k) =
 *                d_uv[t][k], ALWAYS in the caller's triangle order.
 *   Perspective  (CRENDER_TEX_PERSPECTIVE) with z_k the UNPROJECTED z of vertex k:
 *                  q_k = b_k / z_k,   s = (q1 + q2) + q3,
 *                  u = ((u0*q1 + u1*q2) + u2*q3) / s,   and v alike.
 *   Nearest      (default) row = clip(i32((1 - v) * th), 0, th - 1),
 *                          column = clip(i32(u * tw), 0, tw - 1)
 *                — the rule of crender_model_texture_colors (model.py:143-151) — where i32 is the
 *                host's truncating conversion: INT_MIN for a NaN and for anything outside int32.
 *                Colour = the texel's three bytes, each converted to float32.
 *   Bilinear     (CRENDER_TEX_BILINEAR)
 *                  fx = u * tw - 0.5,        fy = (1 - v) * th - 0.5,
 *                  x0 = floor(fx), ax = fx - x0,   y0 = floor(fy), ay = fy - y0,
 *                  columns c0 = clip(i32(x0), 0, tw - 1), c1 = clip(i32(x0 + 1), 0, tw - 1),
 *                  rows    r0 = clip(i32(y0), 0, th - 1), r1 = clip(i32(y0 + 1), 0, th - 1)
 *                (the same i32), and per channel, with t_rc the texel byte at row r, column c as
 *                float32, evaluated left to right:
 *                  (t00 * (1 - ax) + t01 * ax) * (1 - ay) + (t10 * (1 - ax) + t11 * ax) * ay
 *                (t00 = [r0][c0], t01 = [r0][c1], t10 = [r1][c0], t11 = [r1][c1]).  A NaN or infinite
 *                coordinate gives a NaN weight, hence a NaN colour.
 *   Fused light  with d_normal and light3, EVERY pixel of the rows, background included, is then
 *                multiplied by f = clip(s / (m + 1e-6), 0, 1) of its normal (n0, n1, n2):
 *                s = ((0 + n0*l0) + n1*l1) + n2*l2, m = sqrt((n0*n0 + n1*n1) + n2*n2) — bit for bit
 *                this call without a light followed by crender_guro_illumination on the same rows
 *                (guro_illumination.py:20-27), without that pass's 36 bytes per pixel.
 *   Other planes z, normals and the winner plane are only read.
 *
 * No mipmaps: one texel (nearest) or four (bilinear) per pixel, whatever the minification.
 */
#ifndef CRENDER_TEX_H
#define CRENDER_TEX_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of crender_tex_shade */
enum {
    CRENDER_TEX_PERSPECTIVE = 1u,    /* perspective-correct uv (see above); default: affine          */
    CRENDER_TEX_BILINEAR = 2u        /* four texels, edge-clamped; default: the nearest one           */
};

/* Texture the colour plane d_color float32 [H][W][3] over rows y0 <= y < y1.
 *   d_winner   int32 [H][W]: the caller's index of the triangle whose fragment won, -1 = background
 *   d_tri      float32 [T][3][3], UNPROJECTED vertices (may be NULL if T == 0)
 *   d_pos_of   NULL, or uint32 [T]: triangle t sits at d_tri[d_pos_of[t]] (the tile-coherent copy of
 *              crender_plan_set_triangle_order); an entry >= T makes t background
 *   P16        HOST float[16], the projection matrix (crender_projection_matrix)
 *   d_uv       float32 [T][3][2], u and v per corner, in the caller's triangle order (may be NULL if T == 0)
 *   d_texture  uint8 [th][tw][3]
 *   d_normal, light3   both NULL, or the normal plane float32 [H][W][3] and HOST float[3] (l0, l1, l2)
 * CRENDER_EINVAL, before anything touches the device, for: a NULL pointer where one is required,
 * T < 0, th or tw < 1, H or W < 1, rows outside the frame (y0 < 0, y1 > H, y0 >= y1), a light
 * without normals or normals without a light, unknown flag bits.  One launch; no synchronisation. */
CRENDER_API int crender_tex_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                  const float *P16, const float *d_uv, const unsigned char *d_texture, int th,
                                  int tw, const float *d_normal, const float *light3, float *d_color, int H, int W,
                                  int y0, int y1, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_TEX_H */
