/*
 * crender_dof.h — C ABI of the depth-of-field pass of libcrender_hip.so: a gather blur by the circle of confusion
 * the z plane gives.  Same conventions as crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this
 * header: raw device pointers, an int status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work
 * enqueued on `stream` and nothing synchronised.
 */
#ifndef CRENDER_DOF_H
#define CRENDER_DOF_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- Depth of field -------------------------------------------------------------------------------------------------
 * The frame through a lens instead of a pinhole: a post-process that blurs every pixel by its CIRCLE OF CONFUSION, which
 * the z plane gives exactly.  A gather: a pixel sums the colours of the pixels around it, each weighted by how much of its
 * own disc reaches the pixel, so that what is in front spreads over what lies behind it and a blurred background does
 * not bleed over something sharper in front of it.  The colour plane is only read and the result goes to a plane of its
 * own (a pixel reads its neighbours' colours), as crender_wire_edge_aa's.  "ao.h" below is include/crender_ao.h.
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

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_DOF_H */
