/*
 * crender_peel.h — C ABI of transparency of libcrender_hip.so: depth peeling by depth key over the planes a frame
 * left, and the blend of a layer under what is in front of it.  Same conventions as crender_hip.h, whose version
 * number (CRENDER_ABI_VERSION) covers this header: raw device pointers, an int status (CRENDER_OK or a CRENDER_E*
 * code, text in crender_last_error()), work enqueued on `stream` and nothing synchronised.
 */
#ifndef CRENDER_PEEL_H
#define CRENDER_PEEL_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_PEEL_H */
