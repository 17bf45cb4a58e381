/*
 * crender_motion.h — C ABI of the motion passes of libcrender_hip.so: the per-pixel motion vectors of a frame against an
 * earlier pose of the same triangles, and a motion blur that gathers along them.  Same conventions as crender_hip.h,
 * whose version number (CRENDER_ABI_VERSION) covers this header: raw device pointers, an int status (CRENDER_OK or a
 * CRENDER_E* code, text in crender_last_error()), work enqueued on `stream` and nothing synchronised.
 */
#ifndef CRENDER_MOTION_H
#define CRENDER_MOTION_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Arithmetic of both entries: every step below is ONE float32 operation, rounded once, with IEEE division and square
 * root (no contraction into fused multiply-adds, no reciprocal, denormals kept).  No expf, powf or logf.
 *
 * ---- Motion vectors -------------------------------------------------------------------------------------------------
 * The winner plane names every pixel's triangle.  The surface point a pixel shows is carried into the PREVIOUS pose's
 * corners with the rasterizer's own barycentrics, as crender_shadow_shade ("shadow.h" is include/crender_shadow.h)
 * carries it into the light's, and projected with the frame's own matrix: where the point was on the screen.  An exact
 * per-pixel velocity, without finite differences.
 *
 * Result contract of crender_motion_vectors.  For every pixel (x, y) with 0 <= x < W and y0 <= y < y1, d_velocity[y][x]
 * is (+0, +0) unless its winner o = d_winner[y][x] is valid: 0 <= o < T and, with d_pos_of, t = d_pos_of[o] < T
 * (without, t = o).  For a valid winner:
 *   1. triangle t of d_tri is projected as crender_project does, and b1, b2, b3 are its barycentrics at (x, y)
 *      (crender_hip.h, "Barycentrics"), as shadow.h takes them;
 *   2. q_k = b_k / z_k (z_k the UNPROJECTED z of corner k), s = (q1 + q2) + q3;
 *   3. with c_k = d_prev_tri[o][k], per coordinate j:  X_j = ((c_0j * q1 + c_1j * q2) + c_2j * q3) / s
 *      (shadow.h's blend, word for word);
 *   4. if X_2 > 0 is false (behind the camera, or a NaN) the velocity is (+0, +0); otherwise (px, py) is (X_0, X_1, X_2)
 *      projected as crender_project projects a vertex, with P16 and the frame's W and H;
 *   5. vx = ((float)x - px) * exposure, vy = ((float)y - py) * exposure: the pixels the point moved during the
 *      exposure, pointing from where it was to where it is.  If vx or vy is not finite, the velocity is (+0, +0).
 * Rows outside y0 <= y < y1 are not touched; the planes are only read.
 */

/* Write rows y0 <= y < y1 of d_velocity float32 [H][W][2].
 *   d_winner   int32 [H][W]; d_tri float32 [T][3][3], the frame's triangles in the order it was drawn in; d_pos_of NULL
 *              or uint32 [T], where the caller's triangle o sits in d_tri (a presorted frame)
 *   P16        HOST float[16], crender_projection_matrix's
 *   d_prev_tri float32 [T][3][3], the previous pose in the CALLER's triangle order, paired with the frame's triangles
 *              as shadow.h pairs d_ltri
 *   exposure   finite, >= 0: the share of the pose difference the shutter was open for
 *   flags      0
 * CRENDER_EINVAL ("crender_motion_vectors: ..."), before anything is dereferenced or launched, in THIS order: a NULL
 * d_winner, P16 or d_velocity; T < 0; d_tri or d_prev_tri NULL with T > 0; H or W < 1; rows outside the frame; any flag
 * bit; an exposure that is not finite and >= 0.  T == 0 writes zeros.  One launch; no synchronisation. */
CRENDER_API int crender_motion_vectors(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                       const float *P16, const float *d_prev_tri, float exposure, float *d_velocity, int H,
                                       int W, int y0, int y1, unsigned flags, void *stream);

/*
 * ---- Motion blur ----------------------------------------------------------------------------------------------------
 * The reconstruction filter of McGuire, Hennessy, Bukowski and Osman, "A Reconstruction Filter for Plausible Motion
 * Blur" (I3D 2012), with every decision a stated float32 step.  A gather: all pixels of a tile of 32 x 32 walk the same
 * taps, along the tile's DOMINANT velocity, and weigh each by the depths and the velocities of the two pixels.  The colour
 * plane is only read and the result goes to a plane of its own, as crender_dof_blur's ("dof.h" is include/crender_dof.h).
 *
 * Result contract of crender_motion_blur.  Rf = (float)max_radius, N = taps, isoft = 1.0f / soft (once).
 *   Per pixel q of the frame in the rows (a STAGED pixel; no other pixel is ever read):
 *     (vx, vy) = d_velocity[q]; if vx or vy is not finite, (vx, vy) = (0, 0)
 *     hx = vx * 0.5f, hy = vy * 0.5f;   l = sqrtf(hx * hx + hy * hy)           (two products, their sum, the root)
 *     if l > Rf:  k = Rf / l, hx = hx * k, hy = hy * k, l = Rf
 *     il = 1.0f / (l > 0.5f ? l : 0.5f)                              the one division a pixel pays; no tap divides
 *     zv = P14 / (d_z[q] - P10) if 0 <= d_winner[q] < T (d_pos_of is not looked at: dof.h's view depth), otherwise
 *     zv = CRENDER_MOTION_FAR = FLT_MAX (0x7F7FFFFF): finite, equal among background pixels (their difference is 0, never
 *     inf - inf), and farther than every finite view depth by more than any soft the differences below can resolve.
 *   Per tile (32 x 32, tile j of a row of tiles starting at x = 32 j, rows of tiles starting at y0): among the staged
 *     pixels of the tile and of its halo of max_radius on every side, the DOMINANT one has the largest l; among equals,
 *     the first in the frame's row-major order.  D = (hx, hy) of it, after the clamp.  If its l > 0.5f is false, every
 *     pixel of the tile is copied bit for bit.  Otherwise, for i = 0 .. N - 1:
 *       tau = (float)(2 i + 1 - N) / (float)N;   ox = rintf(Dx * tau), oy = rintf(Dy * tau)   (ties to even), each
 *       clamped to -max_radius .. max_radius (which |tau| < 1 makes them anyway);  dist = sqrtf((float)(ox*ox + oy*oy))
 *     A tap with (ox, oy) = (0, 0) is skipped; equal offsets count as often as they occur.
 *   Per pixel p of such a tile and tap i in ascending order, with q = p + (ox, oy): a q off the frame or outside the rows
 *     is skipped.  Otherwise, with m_p = dist * il_p and m_q = dist * il_q:
 *       cone(m) = (t = 1.0f - m) > 0 ? t : 0
 *       cyl(m)  = 1.0f - (u * u) * (3.0f - 2.0f * u),  u = (m - 0.95f) * 10.0f, then u < 0 ? 0 : (u > 1 ? 1 : u)
 *       fg = clamp(1.0f - (zv_q - zv_p) * isoft),  bg = clamp(1.0f - (zv_p - zv_q) * isoft),
 *            clamp(a) = a < 0 ? 0 : (a > 1 ? 1 : a)                  (a NaN stays a NaN)
 *       alpha = (fg * cone(m_q) + bg * cone(m_p)) + 2.0f * (cyl(m_q) * cyl(m_p))
 *     The tap is TAKEN iff alpha > 0 (every NaN fails).
 *   Sums       Sw = il_p, S_j = d_color[p]_j * il_p; per taken tap Sw = Sw + alpha, S_j = S_j + alpha * d_color[q]_j.
 *   Result     a pixel that took no tap: d_out[p] = d_color[p], the bits copied (a -0 and every NaN kept).  Otherwise
 *              d_out[p]_j = S_j / Sw.  Where a NaN or an infinite colour was taken the result may be a NaN: WHICH NaN
 *              (sign, payload) is not stated.
 *   Other planes  only read; d_tri and d_pos_of are never read.  Rows outside y0 <= y < y1 of d_out are not touched.
 *              Nothing is ever read out of bounds, whatever the planes hold.
 *
 * Consequences.  A zero velocity plane, taps == 1 (the one offset is (0, 0)) and a static pose copy the rows.  A static
 * pixel (il = 2) takes no tap from a pixel behind it by soft or more (fg = 0; its own cone and cylinder are 0 from
 * dist = 1 on), nor from another static one: a static surface in front of a moving background keeps its bits.  A pixel
 * moving with half length l spreads over what is behind it at distances dist < l, so below max_radius.  On a frame of
 * one colour a blurred pixel differs from that colour by the rounding of the sums and the quotient only.
 *
 * Not covered: jittered tap positions; radii above CRENDER_MOTION_MAX_RADIUS (the staged tile and its halo, five words a
 * pixel, fill the 64 KB of LDS at 12); velocities of the background.
 */
#define CRENDER_MOTION_MAX_RADIUS 12
#define CRENDER_MOTION_MAX_TAPS 32
#define CRENDER_MOTION_FAR 3.40282346638528859812e+38f

/* Blur rows y0 <= y < y1 of d_color float32 [H][W][3] along d_velocity float32 [H][W][2] into d_out float32 [H][W][3].
 *   d_winner, d_z   int32 / float32 [H][W]; with T the winners say which pixels are covered
 *   d_tri, d_pos_of   accepted (the passes' common frame) and never read; may be NULL
 *   P16        HOST float[16], crender_projection_matrix's
 *   d_color, d_velocity   only read; the velocity may hold anything
 *   max_radius 1 .. CRENDER_MOTION_MAX_RADIUS: the clamp of every half velocity, and the reach of the taps
 *   taps       1 .. CRENDER_MOTION_MAX_TAPS
 *   soft       finite, > 0: the range of view depths over which fg and bg fade
 *   d_out      the result; another plane than d_color
 *   flags      0
 * CRENDER_EINVAL ("crender_motion_blur: ..."), before anything is dereferenced or launched, in THIS order: a NULL d_winner,
 * d_z, P16, d_color, d_velocity or d_out; T < 0; H or W < 1; rows outside the frame; any flag bit; d_out == d_color; a P16
 * that is not of crender_projection_matrix's shape (dof.h's two checks, in its words); max_radius outside 1 .. 12; taps
 * outside 1 .. 32; a soft that is not finite and > 0.  One launch with 5 (32 + 2 max_radius)^2 + 72 words of LDS
 * (62 720 + 288 bytes at 12: below 64 KB, no launch attribute); no synchronisation. */
CRENDER_API int crender_motion_blur(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                    const uint32_t *d_pos_of, const float *P16, const float *d_color,
                                    const float *d_velocity, int max_radius, int taps, float soft, float *d_out, int H, int W,
                                    int y0, int y1, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_MOTION_H */
