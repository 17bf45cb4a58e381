/*
 * crender_ao.h — C ABI of the deferred ambient-occlusion pass of libcrender_hip.so: screen-space ambient
 * occlusion over the z plane, the winner plane and the normal plane a raster launch left (crender_render_model
 * with a d_winner).  Every covered pixel's colour is scaled down by how much nearby geometry — found in the z
 * plane within a pixel radius and within a world radius — rises above its tangent plane.  Same conventions as
 * crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this header as it covers crender_phong.h:
 * raw device pointers, an int status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work
 * enqueued on `stream` and nothing synchronised.
 *
 * Result contract.
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square root
 *                (no contraction into fused multiply-adds, denormals kept).
 *   Constants    computed on the host in double and rounded once to float:
 *                  xs, ys as make_proj computes them: (float)(W / 2.0), (float)(H / 2.0)
 *                  kx = (float)(1.0 / ((double)xs * P16[0])),   ky = (float)(1.0 / ((double)ys * P16[5]))
 *                  r2 = radius * radius                         (in float)
 *                  inv_r2 = (float)(1.0 / ((double)radius * (double)radius))
 *                  inv_n  = (float)(1.0 / n_taps)
 *   Coverage     a pixel q is covered when 0 <= q.x < W, y0 <= q.y < y1 and 0 <= d_winner[q] < T.  Rows
 *                outside the strip hold nothing for this pass.
 *   View depth   zv(q) = P16[14] / (d_z[q] - P16[10]): the z plane holds projected z, and this inverts
 *                crender_project for matrices of crender_projection_matrix's shape.
 *   View point   Q(q) = ( (((float)q.x - xs) * kx) * zv(q),  (((float)q.y - ys) * ky) * zv(q),  zv(q) ).
 *   Centre       for a covered pixel p, Pp = Q(p).  An uncovered pixel is never written.
 *   Normal       default: n = d_normal[p].
 *                CRENDER_AO_FACE_NORMALS: t = d_winner[p], or d_pos_of[t] with a d_pos_of — an entry >= T
 *                  means the pixel is not written; A, B, C the unprojected corners of d_tri[t],
 *                  e1 = B - A, e2 = C - A, g = e1 x e2, each component two products and one subtraction
 *                  (gx = e1y*e2z - e1z*e2y, gy = e1z*e2x - e1x*e2z, gz = e1x*e2y - e1y*e2x);
 *                  s = (gx*Px + gy*Py) + gz*Pz, and if s > 0 then g = -g: g faces the eye at the origin; n = g.
 *                In both cases ln = sqrtf((n0*n0 + n1*n1) + n2*n2) + 1e-6f and nu_c = n_c / ln.
 *   Taps         in order i = 0 .. n_taps-1, from (dx, dy) = taps2[i].  With CRENDER_AO_ROTATE let
 *                r = (p.x & 1) | ((p.y & 1) << 1): r = 0 keeps (dx, dy), r = 1 gives (-dy, dx), r = 2 gives
 *                (dy, -dx), r = 3 gives (-dx, -dy) — exact quarter turns.  q = p + that offset.
 *                If q is not covered, o_i = +0.  Otherwise
 *                  D   = Q(q) - Pp                        (per component)
 *                  dd  = (Dx*Dx + Dy*Dy) + Dz*Dz
 *                  dn  = (Dx*nu0 + Dy*nu1) + Dz*nu2
 *                  c   = dn / sqrtf(dd)
 *                  wgt = 1.0f - dd * inv_r2
 *                  take = dd < r2 && c > min_cos          (both false for every NaN)
 *                  o_i = take ? c * wgt : +0
 *                S = 0, then S = S + o_i for each tap in order.
 *   Result       if !(S > 0) the pixel is NOT written: unoccluded areas keep their bits.  Otherwise
 *                  f = 1.0f - strength * (S * inv_n),   f = f < floor ? floor : f,
 *                and each channel becomes c_i * f.
 *   Other planes z, normals and the winner plane are only read.  Nothing is ever read out of bounds, whatever
 *                the planes hold.
 *
 * Not covered: pixel radii above 32, a blur of the occlusion, bent normals, tap radii scaled by depth, strips
 * that see across their edge.
 */
#ifndef CRENDER_AO_H
#define CRENDER_AO_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRENDER_AO_ROTATE 1u
#define CRENDER_AO_FACE_NORMALS 2u
#define CRENDER_AO_MAX_TAPS 64
#define CRENDER_AO_MAX_RADIUS_PX 32

/* Occlude the colour plane d_color float32 [H][W][3] over rows y0 <= y < y1.
 *   d_winner   int32 [H][W]: the caller's index of the triangle whose fragment won, -1 = background
 *   d_z        float32 [H][W], the z plane of the frame (projected z)
 *   d_tri      float32 [T][3][3], UNPROJECTED camera-frame vertices; read with CRENDER_AO_FACE_NORMALS only
 *   d_pos_of   NULL, or uint32 [T]: triangle t sits at d_tri[d_pos_of[t]]; read with FACE_NORMALS only
 *   P16        HOST float[16], the camera's projection matrix (crender_projection_matrix)
 *   d_normal   float32 [H][W][3], the normal plane of the frame; may be NULL with FACE_NORMALS
 *   taps2      HOST int8 [n_taps][2]: dx, dy
 *   n_taps     1 .. CRENDER_AO_MAX_TAPS
 *   radius_px  1 .. CRENDER_AO_MAX_RADIUS_PX: no tap reaches further in x or in y
 *   radius     the world radius, in the camera frame's units
 *   min_cos    a tap counts when the cosine between the normal and the way to it exceeds this
 *   strength   the factor of the mean occlusion, >= 0
 *   floor      the smallest factor a colour is scaled by, 0 .. 1
 * CRENDER_EINVAL, before anything touches the device, for: a NULL d_winner, d_z, P16, taps2 or d_color;
 * d_normal NULL without FACE_NORMALS; d_tri NULL with FACE_NORMALS and T > 0; T < 0; H or W < 1; rows outside
 * the frame (y0 < 0, y1 > H, y0 >= y1); n_taps outside 1 .. 64; radius_px outside 1 .. 32; a tap with |dx| or
 * |dy| above radius_px, or equal to (0, 0); a radius that is not finite or <= 0; a min_cos, strength or floor
 * that is not finite; strength < 0; floor outside [0, 1]; a P16 the pass cannot invert (any of entries 1, 2, 4,
 * 6, 8, 9, 12, 13 non-zero, or entry 0, 5 or 14 zero or not finite); unknown flag bits.  T == 0 returns
 * CRENDER_OK without a launch.  One launch; no synchronisation. */
CRENDER_API int crender_ao_shade(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                                 const uint32_t *d_pos_of, const float *P16, const float *d_normal,
                                 const int8_t *taps2, int n_taps, int radius_px, float radius, float min_cos,
                                 float strength, float floor, float *d_color, int H, int W, int y0, int y1,
                                 unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_AO_H */
