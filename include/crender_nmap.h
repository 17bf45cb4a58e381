/*
 * crender_nmap.h — C ABI of normal mapping of libcrender_hip.so: a tangent-space map from a height map, and the
 * deferred pass that perturbs the normal plane.  Same conventions as crender_hip.h, whose version number
 * (CRENDER_ABI_VERSION) covers this header: raw device pointers, an int status (CRENDER_OK or a CRENDER_E* code,
 * text in crender_last_error()), work enqueued on `stream` and nothing synchronised.
 */
#ifndef CRENDER_NMAP_H
#define CRENDER_NMAP_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- Normal mapping -------------------------------------------------------------------------------------------------
 * Surface detail below the size of a triangle: a deferred pass that PERTURBS THE NORMAL PLANE of the frame a raster
 * launch left, once and right after the draw.  Everything that lights a pixel afterwards reads that plane —
 * crender_guro_illumination, the fused light of crender_tex_shade / crender_mip_shade / crender_aniso_shade and of
 * crender_ssaa_resolve, crender_phong_shade, crender_ao_shade — and so shows the bumps without a change of its own.
 * "tex.h" and "mip.h" below are include/crender_tex.h and include/crender_mip.h, whose statements are used word for word.
 *
 * A normal map is uint8 [mh][mw][3] in TANGENT SPACE: byte_i = 128 + 127 v_i of a unit vector v = (along u, along v, out
 * of the surface); (128, 128, 255) is "no bump".  Row 0 is the TOP of the image, v = 1, as for a texture.
 *
 * crender_nmap_from_height makes one from a height map, uint8 [mh][mw].  For the texel at (row r, column c), every line
 * ONE float32 operation per operator, rounded once, with IEEE division and square root, no contraction:
 *     k  = scale / 255.0f                                   (once, on the host, in float32)
 *     gx = (float)(h[r][c+1] - h[r][c-1]) * k               (the integer difference, then one conversion)
 *     gy = (float)(h[r-1][c] - h[r+1][c]) * k               (v points up: the row ABOVE minus the row below)
 *     ln = sqrtf((gx*gx + gy*gy) + 1.0f)
 *     vx = -gx / ln,   vy = -gy / ln,   vz = 1.0f / ln
 *     b_i = rintf(v_i * 127.0f + 128.0f)                    (ties to even)
 *     byte_i = !(b_i > 0) ? 0 : (b_i > 255 ? 255 : b_i)     (the clip to 0 .. 255; a NaN, which only an overflowing
 *                                                            scale makes, gives 0)
 * The four neighbours are clamped to the edge (c-1 -> max(c-1, 0), ...), so a 1 x 1 map gives the flat texel; with
 * CRENDER_NMAP_WRAP they wrap around (c-1 -> mw-1 at c = 0, ...).  A flat neighbourhood gives (128, 128, 255).
 */
#define CRENDER_NMAP_WRAP 1u                 /* flag of crender_nmap_from_height: a tiling height map */

/* Fill d_map uint8 [mh][mw][3] from d_height uint8 [mh][mw] (another buffer).
 * CRENDER_EINVAL, before anything is dereferenced or launched, checked in THIS order: a NULL d_height or d_map; mh or mw
 * outside 1 .. 65535; a scale that is not finite; any flag bit but CRENDER_NMAP_WRAP.  One launch; no synchronisation. */
CRENDER_API int crender_nmap_from_height(const uint8_t *d_height, int mh, int mw, float scale, unsigned flags,
                                         uint8_t *d_map, void *stream);

/*
 * Result contract of crender_nmap_shade.  For every pixel (x, y) with y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square root (no
 *                contraction into fused multiply-adds, no reciprocal, denormals kept).  A dot product a.b is
 *                (a0*b0 + a1*b1) + a2*b2 and a length |a| is sqrtf(a.a).
 *   Background   t < 0, t >= T, or d_pos_of[t] >= T: the pixel is not written.  Nothing is ever read out of bounds,
 *                whatever the winner plane holds.
 *   Corners      A, B, C: the three UNPROJECTED vertices of triangle t (d_tri[t], or d_tri[d_pos_of[t]] with a d_pos_of);
 *                (u_k, v_k), k = 0, 1, 2: d_uv[t], indexed by t itself, the caller's order, as in tex.h.
 *   Position     (u, v) at the integer pixel (x, y): Barycentrics, then Affine or (CRENDER_NMAP_PERSPECTIVE) Perspective,
 *                exactly as in tex.h.
 *   Sample       s, float32 [3], of the map at (u, v):
 *                  no filter flag           the texel rule of tex.h (nearest);
 *                  CRENDER_NMAP_BILINEAR    the Bilinear statement of tex.h;
 *                  CRENDER_NMAP_CHAIN       d_map is the mip chain of the mh x mw map in mip.h's layout (crender_mip_build:
 *                                           L = 1 + floor(log2(max(mh, mw))) levels, h_k = max(1, mh >> k), packed
 *                                           tightly), and the sample is mip.h's trilinear one: Neighbours, Footprint and
 *                                           Level word for word (with (th, tw) = (mh, mw)), then a = Bilinear on level
 *                                           l0 and, where f != 0, b = Bilinear on level l0 + 1 and s = a*(1 - f) + b*f,
 *                                           left to right.  The levels are box averages of the BYTES, not re-normalised.
 *   Decode       m_i = (s_i - 128.0f) / 127.0f;  m_i = m_i < -1 ? -1 : m_i      (byte 0 decodes to -1, as byte 1 does)
 *                mx = m_0 * strength,   my = m_1 * strength,   mz = m_2
 *   Tangents     of the TRIANGLE (the frame is per triangle, not smoothed over the mesh):
 *                  e1 = B - A,   e2 = C - A
 *                  du1 = u1 - u0,  dv1 = v1 - v0,  du2 = u2 - u0,  dv2 = v2 - v0
 *                  det = du1*dv2 - du2*dv1,     sg = det < 0 ? -1 : 1
 *                  Tt_j = (e1_j*dv2 - e2_j*dv1) * sg,     Bt_j = (e2_j*du1 - e1_j*du2) * sg       (j = 0, 1, 2)
 *                Tt points along increasing u on the surface, Bt along increasing v (both up to a positive factor).
 *   Frame        around the pixel's STORED normal n = d_normal[y][x]:
 *                  nl = |n|,   Nu = n / nl
 *                  d  = Nu.Tt,   Tp = Tt - Nu*d,   tl = |Tp|,   Tu = Tp / tl
 *                  Bp = (Nu1*Tu2 - Nu2*Tu1,  Nu2*Tu0 - Nu0*Tu2,  Nu0*Tu1 - Nu1*Tu0)
 *                  if (Bp.Bt < 0) Bp = -Bp
 *                The stored normals may point either way relative to the winding: the handedness comes from the uv.
 *   Result       out_j = (Tu_j*mx + Bp_j*my) + Nu_j*mz.  Not normalised: guro_factor divides by the length.  out.Nu = mz
 *                up to rounding, so a bump never turns a normal past 90 degrees.
 *   Write        d_normal[y][x] = out iff
 *                  (det > 0 || det < 0) && nl > 0 && tl > 0 && (mx < 0 || mx > 0 || my < 0 || my > 0)
 *                Every NaN makes the condition false (the last clause is "mx != 0 || my != 0" for numbers).  A flat
 *                texel, strength = 0, a triangle whose uv are degenerate, a zero, NaN or infinite normal, a tangent
 *                parallel to the normal and a sample that is not a number therefore keep the pixel's bits, and with a
 *                finite strength no NaN is ever written.
 *   Other planes d_normal is read and written at (x, y) alone.  z, colours and the winner plane are not among the
 *                arguments; the winner plane, the triangles, the uv and the map are only read.
 *
 * Not covered: per-vertex (smoothed) tangents — a coarse mesh shows facets in the bumps; anisotropic filtering of the
 * map; re-normalised mip levels or variance-to-roughness (Toksvig); parallax or displacement; object-space maps.
 */
enum {
    CRENDER_NMAP_PERSPECTIVE = 1u,   /* perspective-correct uv (tex.h); default: affine                          */
    CRENDER_NMAP_BILINEAR = 2u,      /* four texels (tex.h); default: the nearest one                            */
    CRENDER_NMAP_CHAIN = 4u          /* d_map is a mip chain, the filter is trilinear; not with CRENDER_NMAP_BILINEAR */
};

/* Perturb rows y0 <= y < y1 of the normal plane d_normal float32 [H][W][3].
 *   d_winner, d_tri, T, d_pos_of, P16   as crender_wire_overlay takes them
 *   d_uv       float32 [T][3][2], (u, v) per corner in the CALLER's triangle order (may be NULL if T == 0)
 *   d_map      uint8 [mh][mw][3], or with CRENDER_NMAP_CHAIN the chain of crender_mip_build(map, mh, mw)
 *   mh, mw     the map's size (level 0's), 1 .. 65535
 *   strength   finite; scales the two tangent components of the decoded vector (0: nothing is written)
 * CRENDER_EINVAL, before anything is dereferenced or launched, checked in THIS order: a NULL d_winner, P16, d_map or
 * d_normal; T < 0; T > 0 without d_tri or without d_uv; H or W < 1; rows outside the frame (y0 < 0, y1 > H, y0 >= y1);
 * mh or mw outside 1 .. 65535; a strength that is not finite; an unknown flag bit; CRENDER_NMAP_CHAIN together with
 * CRENDER_NMAP_BILINEAR.  T == 0 returns CRENDER_OK without a launch.  One launch (the chain's level offsets travel in its
 * arguments); no synchronisation. */
CRENDER_API int crender_nmap_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                   const float *P16, const float *d_uv, const uint8_t *d_map, int mh, int mw,
                                   float strength, float *d_normal, int H, int W, int y0, int y1, unsigned flags,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_NMAP_H */
