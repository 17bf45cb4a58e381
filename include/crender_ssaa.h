/*
 * crender_ssaa.h — C ABI of the supersampling resolve of libcrender_hip.so: a frame rendered at s*Ho x s*Wo
 * is averaged over s x s blocks down to Ho x Wo (a box filter), on the device.  Same conventions as
 * crender_tex.h and crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this header too: raw
 * device pointers, an int status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work
 * enqueued on `stream` and nothing synchronised.
 *
 * The pass is bound by memory, so it carries the two passes that would otherwise run over the same bytes: the
 * illumination (crender_guro_illumination, 36 bytes per SOURCE pixel) and the presentation
 * (crender_present_u8, run.py:26's image[::-1].astype('uint8')).
 *
 * Result contract of crender_ssaa_resolve.  H, W are the source frame, Ho = H / s, Wo = W / s.  For every
 * output pixel (X, Y) with Y0 <= Y < Y1 and every channel c:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square
 *                root (no contraction into fused multiply-adds, denormals kept).
 *   Sample       c(j, i) = d_color[Y*s + j][X*s + i][c]   for 0 <= j, i < s.
 *   Fused light  with d_normal and light3, c(j, i) is that value TIMES f = clip(q / (m + 1e-6), 0, 1) of the
 *                normal (n0, n1, n2) = d_normal[Y*s + j][X*s + i]:
 *                  q = ((0 + n0*l0) + n1*l1) + n2*l2,   m = sqrt((n0*n0 + n1*n1) + n2*n2)
 *                (the reduction starts from +0; clip keeps a NaN) — the factor of crender_guro_illumination
 *                (guro_illumination.py:20-27).  Bit for bit crender_guro_illumination over the whole source
 *                frame followed by this call without a light, without that pass's traffic and without
 *                rewriting the source colour plane.
 *   Sum          acc = c(0, 0); then acc = acc + c(j, i) in row-major order, j outer and i inner, skipping
 *                (0, 0).  The sum starts from the first sample, not from 0: s = 1 keeps a -0.  The order is
 *                part of the contract (float32 addition does not associate).
 *   Average      r = acc / (float)(s*s), the correctly rounded quotient.  (For s = 1, 2, 4, 8 the product
 *                with the exact reciprocal is that same quotient.)
 *   float32 out  d_out is float32 [Ho][Wo][3]:  d_out[Y'][X][c] = r, with Y' = Ho - 1 - Y under
 *                CRENDER_SSAA_FLIP, else Y.
 *   uint8 out    (CRENDER_SSAA_U8) d_out is uint8 [Ho][Wo][3]:  d_out[Y'][X][c] = crender_present_u8's cast
 *                of r — truncated toward zero to int32, INT_MIN for a NaN and for anything outside int32,
 *                the low byte kept.
 *   Rows         output rows outside Y0 .. Y1 are not written.
 *   Source       d_color and d_normal are only read.
 *
 * Consequences (tests/test_ssaa_cpu.py asserts them on the host model, tests/test_ssaa_gpu.py on the device):
 *   - s = 1 without flags copies the rows bit for bit (a signalling NaN may come out quiet);
 *   - s = 1 with a light is crender_guro_illumination, written elsewhere;
 *   - s = 1 with CRENDER_SSAA_U8 (| CRENDER_SSAA_FLIP) is crender_present_u8.
 *
 * Not covered: filters other than the box, jittered or rotated sample grids, coverage sampling, and
 * resolving z, normals or the winner plane.
 */
#ifndef CRENDER_SSAA_H
#define CRENDER_SSAA_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of crender_ssaa_resolve */
enum {
    CRENDER_SSAA_U8 = 1u,      /* store uint8 [Ho][Wo][3] instead of float32 [Ho][Wo][3]        */
    CRENDER_SSAA_FLIP = 2u     /* output row Y is stored at row Ho - 1 - Y (run.py:26's [::-1]) */
};
enum { CRENDER_SSAA_MAX = 8 };

/* Resolve rows Y0 <= Y < Y1 of the output from the source colour plane d_color float32 [H][W][3].
 *   d_normal, light3   both NULL, or the source normal plane float32 [H][W][3] and HOST float[3] (l0, l1, l2)
 *   s                  1 .. CRENDER_SSAA_MAX; H and W are multiples of it
 *   d_out              float32 or uint8 [H / s][W / s][3] (flags)
 * CRENDER_EINVAL, before anything touches the device, for: a NULL d_color or d_out, s outside 1 .. 8, H or
 * W < 1 or not a multiple of s, rows outside the output (Y0 < 0, Y1 > H / s, Y0 >= Y1), a light without
 * normals or normals without a light, unknown flag bits.  One launch; no synchronisation. */
CRENDER_API int crender_ssaa_resolve(const float *d_color, const float *d_normal, const float *light3,
                                     int H, int W, int s, int Y0, int Y1,
                                     void *d_out, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_SSAA_H */
