/*
 * crender_phong.h — C ABI of the deferred Phong pass of libcrender_hip.so: per-pixel Blinn-Phong lighting
 * (an ambient term, up to four point or directional lights, a specular term) over the winner plane and
 * the normal plane a raster launch left (crender_render_model with a d_winner).  Same conventions as
 * crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this header as it covers
 * crender_shadow.h: raw device pointers, an int status (CRENDER_OK or a CRENDER_E* code, text in
 * crender_last_error()), work enqueued on `stream` and nothing synchronised.
 * ".pyx" is the reference's crender/cy/pixel_buffer_filler/advanced_pixel_buffer_filler.pyx.
 *
 * Result contract.  For every pixel (x, y) with y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and
 *                square root (no contraction into fused multiply-adds, denormals kept).
 *   Background   t < 0, t >= T, or d_pos_of[t] >= T: the pixel is not written.  Nothing is ever read
 *                out of bounds, whatever the winner plane holds.
 *   Barycentrics exactly as crender_shadow_shade obtains them: the three vertices of triangle t —
 *                d_tri[t], or d_tri[d_pos_of[t]] with a d_pos_of — are projected as crender_project
 *                projects them (.pyx:116-130), and (b1, b2, b3) are the barycentrics of the integer
 *                pixel (x, y) in the projected triangle (math_utils.pyx:8-34).
 *   Surface point P in the camera's frame, ALWAYS perspective-correct.  With z_k the UNPROJECTED z of
 *                corner k and (c0, c1, c2) one coordinate of the triangle's own unprojected corners:
 *                  q_k = b_k / z_k,   s = (q1 + q2) + q3,
 *                  P_c = ((c0*q1 + c1*q2) + c2*q3) / s     for c = x, y and z.
 *   Helpers      len(a)  = sqrtf((a0*a0 + a1*a1) + a2*a2)
 *                g(u, n) = the Guro factor of the normal n under the light u (guro_illumination.py:20-27):
 *                  s = ((0 + n0*u0) + n1*u1) + n2*u2,   f = s / (len(n) + 1e-6f),
 *                  f = f < 0 ? 0 : f,   f = f > 1 ? 1 : f      (two selects: a NaN and a -0 stay)
 *   View vector  the camera is at the origin: V_c = -P_c, Vu_c = V_c / len(V).
 *   Normal       n = d_normal[y][x], the plane the raster stored.
 *   Per light j  in order, j < n_lights, with (x, y, z, kd, ks) = lights5[j]:
 *                  a point light (bit j of directional_mask clear), at (x, y, z) in the camera's frame:
 *                    Lv_c = pos_c - P_c,   Lu_c = Lv_c / len(Lv);
 *                  a directional light (bit j set): Lu = (x, y, z) as given, the unit vector TOWARDS the
 *                    light (the host normalises it);
 *                  d  = g(Lu, n)
 *                  Hv_c = Lu_c + Vu_c,   Hu_c = Hv_c / len(Hv)
 *                  sp = g(Hu, n), then sp = sp * sp repeated shininess_log2 times (the exponent is
 *                    2^shininess_log2: no powf, no logarithm)
 *                  lit = d > 0.  Not lit: d = +0 and sp = +0.  Lit but !(sp > 0): sp = +0.
 *                The negated tests send every NaN to "unlit": a NaN normal, a degenerate triangle, a light
 *                on the surface point or exactly behind the eye leave the ambient term only.
 *   Sums         F  = ambient, then F  = F  + kd_j * d_j   for each light in order;
 *                Ws = 0,       then Ws = Ws + ks_j * sp_j  for each light in order.
 *   Colour       per channel i, with S = spec_color3:
 *                  o = c_i * F + Ws * S_i,   o = o > clamp ? clamp : o,
 *                and the pixel is stored.  With finite colours and coefficients no NaN reaches the
 *                colour plane.
 *   Other planes z, normals and the winner plane are only read.
 *
 * No distance attenuation, no spot cones, no per-light shadows, exponents that are powers of two only.
 */
#ifndef CRENDER_PHONG_H
#define CRENDER_PHONG_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CRENDER_PHONG_MAX_LIGHTS 4
#define CRENDER_PHONG_MAX_SHININESS_LOG2 12

/* Light the colour plane d_color float32 [H][W][3] over rows y0 <= y < y1.
 *   d_winner   int32 [H][W]: the caller's index of the triangle whose fragment won, -1 = background
 *   d_tri      float32 [T][3][3], UNPROJECTED camera-frame vertices (may be NULL if T == 0)
 *   d_pos_of   NULL, or uint32 [T]: triangle t sits at d_tri[d_pos_of[t]] (the tile-coherent copy of
 *              crender_plan_set_triangle_order); an entry >= T makes t background
 *   P16        HOST float[16], the camera's projection matrix (crender_projection_matrix)
 *   d_normal   float32 [H][W][3], the normal plane of the frame
 *   lights5    HOST float[n_lights][5]: x, y, z, kd, ks
 *   n_lights   1 .. CRENDER_PHONG_MAX_LIGHTS
 *   directional_mask   bit j: light j is a direction, not a position
 *   ambient    added to the diffuse factor of every covered pixel, >= 0
 *   shininess_log2     the specular exponent is 2^shininess_log2; 0 .. CRENDER_PHONG_MAX_SHININESS_LOG2
 *   spec_color3        HOST float[3], the colour of the highlight
 *   clamp      the largest value a channel is stored with; +inf = none
 *   flags      0
 * CRENDER_EINVAL, before anything touches the device, for: a NULL pointer where one is required,
 * T < 0, H or W < 1, rows outside the frame (y0 < 0, y1 > H, y0 >= y1), n_lights outside 1 .. 4, mask bits
 * at or above n_lights, shininess_log2 outside 0 .. 12, an ambient, kd, ks, light vector or spec_color3 that
 * is not finite, an ambient, kd or ks that is negative, a clamp that is NaN, any flag bit.  T == 0 returns
 * CRENDER_OK without a launch.  One launch; no synchronisation. */
CRENDER_API int crender_phong_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                    const float *P16, const float *d_normal, const float *lights5, int n_lights,
                                    unsigned directional_mask, float ambient, int shininess_log2,
                                    const float *spec_color3, float clamp, float *d_color, int H, int W, int y0, int y1,
                                    unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_PHONG_H */
