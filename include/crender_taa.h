/*
 * crender_taa.h — C ABI of the temporal anti-aliasing resolve of libcrender_hip.so: a frame drawn with a sub-pixel
 * offset blended into a history image that follows the surface across the screen.  Same conventions as crender_hip.h,
 * whose version number (CRENDER_ABI_VERSION) covers this header and STAYS what it was (the change is additive): raw
 * device pointers, an int status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work enqueued on
 * `stream` and nothing synchronised.
 */
#ifndef CRENDER_TAA_H
#define CRENDER_TAA_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Arithmetic: every step below is ONE float32 operation, rounded once (no contraction into fused multiply-adds,
 * denormals kept).  The entry divides nowhere and takes no root.
 *
 * Result contract of crender_taa_resolve, for every pixel p = (x, y) with 0 <= x < W and y0 <= y < y1.  N(p) is the set
 * of up to nine pixels (x + dx, y + dy), dx, dy in {-1, 0, 1}, that lie on the frame AND in the rows (the strip does not
 * see across its edge), visited in row-major order (dy = -1 first, within a row dx = -1 first).  keep = 1.0f - blend,
 * computed once.  c = d_color[p].
 *   1. Velocity.  (vx, vy) = (0, 0) without d_velocity.  Otherwise it is d_velocity[s]: s = p without d_z; with d_z,
 *      start from best = d_z[p] and s = p, visit N(p) and replace both on d_z[n] < best: p wins ties, then the first
 *      neighbour in order, and a NaN never replaces (the velocity of the nearest surface of the 3 x 3: "dilated").  If
 *      vx or vy is not finite, (vx, vy) = (0, 0).
 *   2. Where it was.  px = (float)x - vx, py = (float)y - vy.  The history counts iff
 *        px >= 0 && px <= (float)(W - 1) && py >= (float)y0 && py <= (float)(y1 - 1).
 *      If it does not, d_out[p] = c, the bits copied.
 *   3. History sample.  x0 = floorf(px), fx = px - x0, ix0 = (int)x0, ix1 = min(ix0 + 1, W - 1); y0' = floorf(py),
 *      fy = py - y0', iy0 = (int)y0', iy1 = min(iy0 + 1, y1 - 1).  With h00 = d_history[iy0][ix0], h01 = [iy0][ix1],
 *      h10 = [iy1][ix0], h11 = [iy1][ix1], per channel:
 *        top = fx == 0 ? h00 : h00 + (h01 - h00) * fx;   bot = fx == 0 ? h10 : h10 + (h11 - h10) * fx;
 *        h   = fy == 0 ? top : top + (bot - top) * fy.
 *      A tap of weight zero never reaches the result (a NaN there is not seen).
 *   4. Neighbourhood box, skipped with CRENDER_TAA_NO_CLAMP (hc = h).  Per channel lo = hi = c; over N(p) with
 *      v = d_color[n]:  if (v < lo) lo = v;  if (v > hi) hi = v;  then  hc = h < lo ? lo : (h > hi ? hi : h).  A NaN h
 *      stays a NaN.
 *   5. Blend.  d_out[p] = c + (hc - c) * keep: three operations per channel.  Where a NaN or an infinity entered, the
 *      result may be a NaN whose sign and payload are not stated.
 * blend == 1 is decided on the host and copies the rows of d_color bit for bit.  The planes are only read; rows outside
 * y0 <= y < y1 of d_out are not touched; nothing is ever read out of bounds, whatever the planes hold.
 *
 * Consequences.  With finite inputs and blend < 1 the clamped result lies in [lo, hi] up to the rounding of step 5's
 * three operations, so a history that has nothing to do with the frame cannot leave the colours of the 3 x 3.  A zero
 * velocity reads one history texel per pixel.  A history equal to the frame returns the frame (hc - c = 0).
 *
 * Traffic per pixel, counted from the kernel: a tile of 32 x 32 stages (34 / 32)^2 = 1.13 times its own pixels, so 13.5 B
 * of colour, and with a velocity 9.0 B of it, with d_z 4.5 B more; the history is one texel of 12 B, or four (48 B asked,
 * mostly shared between neighbours in the caches: about 12 B of new lines); 12 B are stored.  37.5 B a pixel for a static
 * view, 51 B with velocity and dilation.
 *
 * Not covered: variance clipping, a YCoCg box, history rejection by depth or winner, sharpening, un-jittering the
 * current sample.
 */
#define CRENDER_TAA_NO_CLAMP 1u

/* Resolve rows y0 <= y < y1 of d_color float32 [H][W][3] against d_history float32 [H][W][3] into d_out float32 [H][W][3].
 *   d_velocity NULL (a static view) or float32 [H][W][2], crender_motion_vectors' plane: the pixels a surface point moved
 *              since the history's frame, pointing from where it was to where it is; it may hold anything
 *   d_z        NULL or float32 [H][W], the frame's z plane (smaller is nearer): the velocity is taken from the nearest
 *              pixel of the 3 x 3.  Only with d_velocity
 *   blend      in (0, 1]: the share of the new frame
 *   d_out      the result; another plane than d_color and d_history
 *   flags      0 or CRENDER_TAA_NO_CLAMP
 * CRENDER_EINVAL ("crender_taa_resolve: ..."), before anything is dereferenced or launched, in THIS order: a NULL d_color,
 * d_history or d_out; d_z without d_velocity; H or W < 1; rows outside the frame; an unknown flag bit; d_out equal to
 * d_color or d_history; a blend that is not finite or not in (0, 1].  One launch (blend == 1: one copy) with 3 to 6 planes
 * of 34 x 34 words of LDS (13 872 to 27 744 bytes: no launch attribute); no synchronisation. */
CRENDER_API int crender_taa_resolve(const float *d_color, const float *d_history, const float *d_velocity, const float *d_z,
                                    float blend, float *d_out, int H, int W, int y0, int y1, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_TAA_H */
