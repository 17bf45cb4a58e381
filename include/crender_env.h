/*
 * crender_env.h — C ABI of the environment pass of libcrender_hip.so: cube-map reflections and a skybox over the
 * winner plane.  Same conventions as crender_hip.h, whose version number (CRENDER_ABI_VERSION) covers this header:
 * raw device pointers, an int status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work enqueued
 * on `stream` and nothing synchronised.
 */
#ifndef CRENDER_ENV_H
#define CRENDER_ENV_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- Environment mapping --------------------------------------------------------------------------------------------
 * What is around the model: a deferred pass that looks a DIRECTION up in a cube map, for the covered pixels the
 * direction in which the surface mirrors the eye (reflections), for the others the pixel's own view ray (a skybox).
 * Everything it needs is resident after a frame: the winner plane and the triangles give the surface point, exactly as
 * crender_phong_shade rebuilds it, the normal plane — perturbed by crender_nmap_shade or not — the normal, the
 * projection a background pixel's ray.
 * "tex.h", "phong.h" and "ao.h" below are include/crender_tex.h, crender_phong.h and crender_ao.h, whose statements are
 * used word for word.
 *
 * Result contract of crender_env_shade.  For every pixel (x, y) with 0 <= x < W, y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square root (no
 *                contraction into fused multiply-adds, no reciprocal, denormals kept).  Constants named "host" are
 *                computed in double and rounded once to float.
 *   Frames       the camera's frame is the rasterizer's: x grows with the column, y with the row, z goes into the screen,
 *                the eye is at the origin.  The environment's frame is the camera's turned by M (below).
 *   Environment  a cube map uint8 [6][S][S][3], 1 <= S <= CRENDER_ENV_MAX_SIDE, the faces in the order +x, -x, +y, -y,
 *                +z, -z of the environment's frame.  The +z face is what the camera itself sees (under the identity);
 *                the others are that frame turned by quarter turns.  Row 0 of a face is where tc (below) is smallest.
 *   Face         of a direction d: a = (|d0|, |d1|, |d2|); the major axis is x if a0 >= a1 && a0 >= a2, else y if
 *                a1 >= a2, else z (so a NaN falls through to z); ma is that magnitude, face = 2 axis + (d_axis < 0), and
 *                    face   +x    -x    +y    -y    +z    -z
 *                    sc    -d2    d2    d0    d0    d0   -d0
 *                    tc     d1    d1   -d2    d2    d1    d1
 *                d is USABLE when ma > 0 && ma < INFINITY.  A pixel whose direction is not usable is not written.
 *   Sample       e = the Bilinear statement of tex.h, unchanged, on that face taken as an S x S texture, at
 *                    tu = (sc / ma + 1.0f) * 0.5f,     tv = (1.0f - tc / ma) * 0.5f
 *                (the row grows with tc; indices are clamped to the face: nothing is filtered across faces).
 *   Two levels   with d_faces1 (side S1) and 0 < level_frac = f < 1: e_c = e0_c * (1.0f - f) + e1_c * f, both levels
 *                sampled at the same direction.  Which two levels of a chain they are is the host's matter.
 *   Orientation  M9 is a row-major 3 x 3: d_i = (M[i][0]*r0 + M[i][1]*r1) + M[i][2]*r2.
 *
 *   CRENDER_ENV_REFLECT, for a COVERED pixel (0 <= t < T and, with a d_pos_of, d_pos_of[t] < T), unless reflectivity == 0
 *   (then no covered pixel is written):
 *     Point      p: project the winner, the rasterizer's barycentrics b_k, then phong.h's "Surface point":
 *                    q_k = b_k / z_k,   s = (q1 + q2) + q3,   p_c = ((A_c*q1 + B_c*q2) + C_c*q3) / s
 *     Mirror     n = d_normal[y][x];  nn = (n0*n0 + n1*n1) + n2*n2,  ni = (n0*p0 + n1*p1) + n2*p2,
 *                    k = (2.0f * ni) / nn,      r_c = p_c - k * n_c
 *                (not normalised: the face and the two quotients do not depend on |r|; and the same for n and -n).
 *                d = M r, e the sample.
 *     Weight     pp = (p0*p0 + p1*p1) + p2*p2,   c = fabsf(ni) / (sqrtf(nn) * sqrtf(pp)),   m = 1.0f - c,
 *                    m = m < 0 ? 0 : m,   m = m > 1 ? 1 : m;   a NaN m makes the pixel NOT written
 *                    m5 = ((m*m) * (m*m)) * m,     w = reflectivity * (f0 + one_minus_f0 * m5)
 *                with host one_minus_f0 = (float)(1.0 - (double)f0): Schlick's weight, f0 facing the eye, 1 at a
 *                grazing angle.
 *     Result     colour_c = colour_c * (1.0f - w) + (e_c * tint_c) * w
 *
 *   CRENDER_ENV_BACKGROUND, for every pixel of the rows that is NOT covered (winners that name no triangle included):
 *     Ray        with ao.h's host constants xs, ys, kx, ky: r = (((float)x - xs) * kx, ((float)y - ys) * ky, 1.0f)
 *                d = M r, e the sample.
 *     Result     colour_c = e_c * background_gain
 *
 *   Other planes z, normals and the winner plane are only read.  Nothing is ever read out of bounds, whatever the
 *                planes hold.
 *
 * Not covered: filtering across the seams of the faces; prefiltered (cosine or GGX) chains — two levels are a blur, not
 * a roughness model —; per-pixel reflectivity; refraction; diffuse irradiance; reflections that see the model itself.
 */
#define CRENDER_ENV_REFLECT 1u               /* covered pixels mirror the environment                                   */
#define CRENDER_ENV_BACKGROUND 2u            /* the other pixels of the rows show it                                    */
#define CRENDER_ENV_MAX_SIDE 8192

/* Shade rows y0 <= y < y1 of the colour plane d_color float32 [H][W][3].
 *   d_winner, d_tri, T, d_pos_of, P16   as crender_wire_overlay takes them; d_tri is read with REFLECT only
 *   d_normal   float32 [H][W][3], the normal plane of the frame; may be NULL without REFLECT
 *   d_faces0   uint8 [6][S0][S0][3]
 *   d_faces1   NULL, or uint8 [6][S1][S1][3]: the second level
 *   level_frac the weight of the second level, 0 < level_frac < 1; 0 without one
 *   M9         HOST float[9], finite: the orientation
 *   reflectivity, f0   0 .. 1
 *   tint3      HOST float[3], finite: a factor per channel of the reflected sample
 *   background_gain    finite, >= 0
 *   flags      CRENDER_ENV_REFLECT, CRENDER_ENV_BACKGROUND or both
 * CRENDER_EINVAL ("crender_env_shade: ..."), before anything is dereferenced or launched, checked in THIS order: a NULL
 * d_winner, P16, d_faces0, M9, tint3 or d_color, or a NULL d_normal with REFLECT; T < 0; T > 0 without d_tri; H or W < 1;
 * rows outside the frame (y0 < 0, y1 > H, y0 >= y1); S0 outside 1 .. 8192 or S1 outside 0 .. 8192; d_faces1, S1 and
 * level_frac that are neither all given (S1 >= 1, 0 < level_frac < 1) nor all absent (NULL, 0, 0); an M9, tint3 or
 * background_gain that is not finite, a reflectivity or f0 outside [0, 1], a negative background_gain; with BACKGROUND a
 * P16 whose entry 0 or 5 is zero or not finite; an unknown flag bit, or neither flag.  With REFLECT alone T == 0 and
 * reflectivity == 0 return CRENDER_OK without a launch; with BACKGROUND T == 0 paints every pixel of the rows.  One
 * launch (M9, tint3 and the coefficients travel in its arguments); no synchronisation. */
CRENDER_API int crender_env_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                  const float *P16, const float *d_normal, const uint8_t *d_faces0, int S0,
                                  const uint8_t *d_faces1, int S1, float level_frac, const float *M9, float reflectivity,
                                  float f0, const float *tint3, float background_gain, float *d_color, int H, int W,
                                  int y0, int y1, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_ENV_H */
