/*
 * crender_shadow.h — C ABI of the deferred shadow pass of libcrender_hip.so: shadow mapping over the
 * winner plane a raster launch left (crender_render_model with a d_winner), with the z plane (and,
 * optionally, the winner plane) of a SECOND frame — the same triangles rendered from the light — as
 * the shadow map.  Same conventions as crender_hip.h, whose version number (CRENDER_ABI_VERSION)
 * covers this header as it covers crender_tex.h: raw device pointers, an int status (CRENDER_OK or a
 * CRENDER_E* code, text in crender_last_error()), work enqueued on `stream` and nothing synchronised.
 * ".pyx" is the reference's crender/cy/pixel_buffer_filler/advanced_pixel_buffer_filler.pyx.
 *
 * Result contract.  For every pixel (x, y) with y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division
 *                (no contraction into fused multiply-adds, denormals kept).
 *   Background   t < 0, t >= T, or d_pos_of[t] >= T: the colour is left as it is.  Nothing is ever
 *                read out of bounds, whatever either winner plane holds.
 *   Barycentrics exactly as crender_tex_shade obtains them: the three vertices of triangle t —
 *                d_tri[t], or d_tri[d_pos_of[t]] with a d_pos_of — are projected as crender_project
 *                projects them (.pyx:116-130), and (b1, b2, b3) are the barycentrics of the integer
 *                pixel (x, y) in the projected triangle (math_utils.pyx:8-34).
 *   Surface point in the light's frame, ALWAYS perspective-correct (an affine blend of the corners is
 *                not the point of the surface the pixel shows).  With z_k the UNPROJECTED camera z of
 *                corner k and (c0, c1, c2) one coordinate of the three corners of d_ltri[t] — the
 *                CALLER'S index t, whatever d_pos_of says:
 *                  q_k = b_k / z_k,   s = (q1 + q2) + q3,
 *                  c = ((c0*q1 + c1*q2) + c2*q3) / s     for c = X, Y and Z.
 *   Into the map (X, Y, Z) goes through the statements of crender_project for one vertex with PL16,
 *                Wl and Hl — the in-place column quirk included (.pyx:116-130: column j is formed from
 *                the columns before it as already overwritten) — which gives (sx, sy, sz).  The filler
 *                samples at integer coordinates, so the texel is
 *                  cx = i32(floor(sx + 0.5)),   cy = i32(floor(sy + 0.5)),
 *                where i32 is the host's truncating conversion: INT_MIN for a NaN and for anything
 *                outside int32.
 *   Taps         r = (K - 1) / 2 with K = pcf.  Tap (i, j), i and j in [-r, r], looks at column cx + i
 *                and row cy + j; the sums are evaluated without int32 overflow.
 *   A tap is LIT when any of these holds, else it is shadowed:
 *                  !(Z > 0)                                  behind the light, or NaN;
 *                  the tap is outside [0, Wl) x [0, Hl);
 *                  d_lwinner is given and d_lwinner[row][col] == t   the light sees this very triangle
 *                                                            there: lit without any depth bias;
 *                  !(sz - bias > d_lz[row][col]).
 *                The negated forms make every NaN lit.  n is the number of lit taps.
 *   Colour       n == K*K: the pixel is NOT WRITTEN, so lit areas keep their bits.  Otherwise
 *                  frac = float(n) / float(K*K),  om = 1 - ambient,  m = om * frac,  f = ambient + m,
 *                and each of the three channels is multiplied by f.
 *   Other planes z, normals and both winner planes are only read.
 *
 * One light per call, a perspective light only; no cascades, no slope-scaled bias, box weights.
 */
#ifndef CRENDER_SHADOW_H
#define CRENDER_SHADOW_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Shadow the colour plane d_color float32 [H][W][3] over rows y0 <= y < y1.
 *   d_winner   int32 [H][W]: the caller's index of the triangle whose fragment won, -1 = background
 *   d_tri      float32 [T][3][3], UNPROJECTED camera-frame vertices (may be NULL if T == 0)
 *   d_pos_of   NULL, or uint32 [T]: triangle t sits at d_tri[d_pos_of[t]] (the tile-coherent copy of
 *              crender_plan_set_triangle_order); an entry >= T makes t background
 *   P16        HOST float[16], the camera's projection matrix (crender_projection_matrix)
 *   d_ltri     float32 [T][3][3], UNPROJECTED light-frame vertices in the CALLER'S triangle order,
 *              like crender_tex_shade's d_uv (may be NULL if T == 0)
 *   PL16       HOST float[16], the light's projection matrix
 *   d_lz       float32 [Hl][Wl], the z plane of the light's frame
 *   d_lwinner  NULL, or int32 [Hl][Wl], the winner plane of the light's frame (caller's indices)
 *   bias       subtracted from the pixel's depth in the light's projected z before the comparison
 *   ambient    the factor of a fully shadowed pixel, in [0, 1]
 *   pcf        K: the taps are the K x K texels around the pixel's; 1, 3 or 5
 *   flags      0
 * CRENDER_EINVAL, before anything touches the device, for: a NULL pointer where one is required,
 * T < 0, H, W, Hl or Wl < 1, rows outside the frame (y0 < 0, y1 > H, y0 >= y1), pcf not 1, 3 or 5,
 * ambient outside [0, 1] or NaN, a bias that is not finite, any flag bit.  T == 0 returns CRENDER_OK
 * without a launch.  One launch; no synchronisation. */
CRENDER_API int crender_shadow_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                     const float *P16, const float *d_ltri, const float *PL16, const float *d_lz,
                                     const int32_t *d_lwinner, int Hl, int Wl, float bias, float ambient, int pcf,
                                     float *d_color, int H, int W, int y0, int y1, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_SHADOW_H */
