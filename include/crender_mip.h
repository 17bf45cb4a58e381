/*
 * crender_mip.h — C ABI of the mip chain and the trilinear texture pass of libcrender_hip.so: what
 * crender_tex.h leaves open ("No mipmaps").  Same conventions as crender_tex.h and crender_hip.h, whose
 * version number (CRENDER_ABI_VERSION) covers this header too: raw device pointers, an int status
 * (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work enqueued on `stream` and nothing
 * synchronised.  "tex.h" below is include/crender_tex.h.
 *
 * Chain.  A th x tw texture (uint8, three channels) has
 *     L = 1 + floor(log2(max(th, tw)))
 * levels: (h_0, w_0) = (th, tw), then h_k = max(1, h_{k-1} >> 1) and w_k alike.  The levels are packed
 * tightly in order: level k starts at byte 3 * sum_{i<k} h_i * w_i and is uint8 [h_k][w_k][3].  Level 0 is
 * the texture.  Texel (r, c), channel j of level k, in integer arithmetic over level k - 1 (height h,
 * width w):
 *     (A + B + C + D + 2) >> 2
 * with A, B, C, D the texels at rows min(2r, h - 1), min(2r + 1, h - 1) x columns min(2c, w - 1),
 * min(2c + 1, w - 1).  L <= CRENDER_MIP_MAX_LEVELS: a side above 65 535 is refused.
 *
 * Result contract of crender_mip_shade.  For every pixel (x, y) with y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square
 *                root (no contraction into fused multiply-adds, denormals kept).
 *   Background, Barycentrics, Affine, Perspective
 *                exactly as in tex.h (d_pos_of included), giving (u, v) at the integer pixel (x, y).
 *   Neighbours   the same chain — barycentrics of triangle t, then Affine or Perspective — is evaluated at
 *                the integer pixels (x + 1, y), giving (ux, vx), and (x, y + 1), giving (uy, vy).  This is
 *                arithmetic alone: no plane is read there, so those pixels may lie outside the triangle,
 *                the rows or the frame.
 *   Footprint    with tw and th converted to float32:
 *                  dudx = (ux - u) * tw,   dvdx = (vx - v) * th,
 *                  dudy = (uy - u) * tw,   dvdy = (vy - v) * th,
 *                  rx = dudx*dudx + dvdx*dvdx,   ry = dudy*dudy + dvdy*dvdy,
 *                  r2 = (rx >= ry) ? rx : ry          (a NaN rx gives ry, a NaN ry gives NaN)
 *                  rho = sqrt(r2)
 *   Level        by comparisons, never by a logarithm (log2f is not reproducible between host and device):
 *                  !(rho > 1)            (magnification, or NaN)                 l0 = 0,     f = 0
 *                  else !(rho < 2^(L-1)) (+inf included; always so when L = 1)   l0 = L - 1, f = 0
 *                  else rho = m * 2^(e+1) with 0.5 <= m < 1 (frexp, exact):      l0 = e,
 *                       f = rho / 2^e - 1      (one exact scaling, one subtraction; 0 <= f < 1)
 *                f stands in, piecewise linearly, for the fractional part of log2(rho).
 *   Colour       a = the Bilinear statement of tex.h applied to level l0, with (th, tw) replaced by
 *                (h_l0, w_l0).  If f == 0 the colour is a.  Otherwise b is the same on level l0 + 1 and, per
 *                channel, the colour is  a * (1 - f) + b * f  evaluated left to right.
 *   Fused light, Other planes
 *                word for word as in tex.h.
 *
 * Not covered here: anisotropic filtering (a surface seen at a grazing angle takes the level of its longer
 * axis, and blurs along the shorter) is include/crender_aniso.h's crender_aniso_shade, on this chain;
 * nearest-within-level filters.
 */
#ifndef CRENDER_MIP_H
#define CRENDER_MIP_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CRENDER_MIP_MAX_LEVELS = 16 };

/* flags of crender_mip_shade */
enum {
    CRENDER_MIP_PERSPECTIVE = 1u     /* perspective-correct uv (tex.h); default: affine               */
};

/* The chain's shape, on the host (no GPU is touched).  Every output pointer may be NULL.
 *   levels       *levels = L
 *   h16, w16     int [CRENDER_MIP_MAX_LEVELS]: h_k, w_k for k < L, 0 beyond
 *   offset16     uint64 [CRENDER_MIP_MAX_LEVELS]: the byte at which level k starts, 0 beyond
 *   total_bytes  the size of the whole chain
 * CRENDER_EINVAL for th or tw < 1 and for a side above 65 535 (L > 16). */
CRENDER_API int crender_mip_layout(int th, int tw, int *levels, int *h16, int *w16, uint64_t *offset16,
                                   uint64_t *total_bytes);

/* Fill d_chain (crender_mip_layout's total_bytes) from d_texture uint8 [th][tw][3]: one copy for level 0,
 * then one launch per level, each reading the level before it.  d_chain must not overlap d_texture.
 * CRENDER_EINVAL for a NULL pointer and for what crender_mip_layout refuses.  No synchronisation. */
CRENDER_API int crender_mip_build(const unsigned char *d_texture, int th, int tw, unsigned char *d_chain,
                                  void *stream);

/* crender_tex_shade with trilinear filtering: its arguments, with the chain of the th x tw texture
 * (crender_mip_build) in place of the texture.  CRENDER_EINVAL, before anything touches the device, for
 * the argument errors of crender_tex_shade (unknown flag bits among them: CRENDER_MIP_PERSPECTIVE is
 * the only flag) and for a side above 65 535.  One launch; no synchronisation. */
CRENDER_API int crender_mip_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                  const float *P16, const float *d_uv, const unsigned char *d_chain, int th,
                                  int tw, const float *d_normal, const float *light3, float *d_color, int H, int W,
                                  int y0, int y1, unsigned flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_MIP_H */
