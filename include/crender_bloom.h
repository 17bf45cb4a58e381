/*
 * crender_bloom.h — C ABI of bloom and tone mapping of libcrender_hip.so: a separable glow pass and a tone curve over
 * any float32 image.  Same conventions as crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this
 * header: raw device pointers, an int status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work
 * enqueued on `stream` and nothing synchronised.
 */
#ifndef CRENDER_BLOOM_H
#define CRENDER_BLOOM_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- Bloom ----------------------------------------------------------------------------------------------------------
 * Bloom and tone mapping: a glow around what is brighter than a threshold, and a curve that brings the range back into
 * 0 .. 255.  A post-process over ANY float32 image [H][W][3] — the filler's colour plane, or the tensor of
 * crender_wire_edge_aa, crender_dof_blur, crender_peel_blend or crender_ssaa_resolve — and so the first stage that can
 * follow any of them.  The blur is SEPARABLE: the rows into a scratch plane, then the columns.
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
#endif /* CRENDER_BLOOM_H */
