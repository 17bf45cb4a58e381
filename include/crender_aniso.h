/*
 * crender_aniso.h — C ABI of the anisotropic texture pass of libcrender_hip.so: what crender_mip.h leaves
 * open ("Not covered: anisotropic filtering").  Same conventions as crender_mip.h and crender_hip.h, whose
 * version number (CRENDER_ABI_VERSION) covers this header too: raw device pointers, an int status (CRENDER_OK
 * or a CRENDER_E* code, text in crender_last_error()), work enqueued on `stream` and nothing synchronised.
 * "mip.h" below is include/crender_mip.h; the chain is the one crender_mip_build fills.
 *
 * Trilinear filtering takes the level of the LONGER of a pixel's two texel-space steps, so a surface seen at
 * a grazing angle is blurred along its shorter one.  Here the level comes from the SHORTER step, widened until
 * the ratio of the two is at most A = max_aniso and never below one texel, and N <= A trilinear samples,
 * equally weighted, span the longer step.
 *
 * Result contract of crender_aniso_shade.  For every pixel (x, y) with y0 <= y < y1 and t = d_winner[y][x]:
 *
 *   Arithmetic   every step below is ONE float32 operation, rounded once, with IEEE division and square
 *                root (no contraction into fused multiply-adds, denormals kept).
 *   Background, Barycentrics, Affine, Perspective, Neighbours
 *                exactly as in mip.h, giving (u, v) at (x, y), (ux, vx) at (x + 1, y), (uy, vy) at (x, y + 1).
 *   Axes         with tw and th converted to float32:
 *                  dux = ux - u,      dvx = vx - v,      duy = uy - u,      dvy = vy - v,
 *                  dudx = dux * tw,   dvdx = dvx * th,   dudy = duy * tw,   dvdy = dvy * th,
 *                  rx = dudx*dudx + dvdx*dvdx,   ry = dudy*dudy + dvdy*dvdy      (the bits of mip.h's Footprint)
 *                The major axis is x if rx >= ry, else y (a NaN rx makes y the major axis).  r2max and r2min
 *                are the major and the minor squared length, pmax = sqrt(r2max), pmin = sqrt(r2min), and
 *                (du, dv) is the major axis's pair of differences: (dux, dvx) or (duy, dvy).
 *   Footprint and sample count, with A converted to float32:
 *                  !(pmax > 1)   (magnification, or NaN)      N = 1,  rho = pmax
 *                  else  lo  = pmax / A
 *                        rho = (pmin >= lo) ? pmin : lo       (a NaN pmin gives lo)
 *                        rho = (rho >= 1) ? rho : 1
 *                        q   = pmax / rho
 *                        !(q > 1)                             N = 1
 *                        else nf = ceilf(q),                  N = (nf < A) ? (int)nf : A
 *   Level        mip.h's Level applied to this rho gives l0 and f, once per pixel.
 *   Colour       If N == 1: mip.h's Colour at (u, v); no offset is formed (du * 0 is NaN for an infinite du).
 *                Otherwise, for i = 0 .. N - 1:
 *                  o_i = (float)(2*i + 1 - N) / (float)(2*N)
 *                  u_i = u + du * o_i,   v_i = v + dv * o_i          (a product, then a sum)
 *                  c_i = mip.h's Colour at (u_i, v_i) with the pixel's l0 and f
 *                and per channel s = ((c_0 + c_1) + c_2) + ... in order; the colour is s / (float)N.
 *   Fused light, Other planes
 *                word for word as in mip.h.
 *
 * Consequences (tests/test_aniso_cpu.py asserts them on the host model):
 *   - with max_aniso = 1 every pixel is crender_mip_shade's pixel, bit for bit (lo = pmax, so rho = pmax);
 *   - every pixel with N == 1 is crender_mip_shade's pixel, bit for bit;
 *   - l0 never exceeds crender_mip_shade's l0;
 *   - l0 is never below crender_mip_shade's l0 minus ceil(log2(max_aniso)).
 *
 * Not covered: elliptical (EWA) weighting of the samples, anisotropy for the filters without a chain.
 */
#ifndef CRENDER_ANISO_H
#define CRENDER_ANISO_H

#include "crender_mip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { CRENDER_ANISO_MAX = 16 };

/* crender_mip_shade with up to max_aniso samples along each pixel's major axis: its arguments, then
 * max_aniso (1 .. CRENDER_ANISO_MAX).  `flags` accepts CRENDER_MIP_PERSPECTIVE only.  CRENDER_EINVAL, before
 * anything touches the device, for the argument errors of crender_mip_shade and for max_aniso outside
 * 1 .. 16.  T == 0 without a light is CRENDER_OK with nothing launched.  One launch; no synchronisation. */
CRENDER_API int crender_aniso_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                                    const float *P16, const float *d_uv, const unsigned char *d_chain, int th,
                                    int tw, const float *d_normal, const float *light3, float *d_color, int H, int W,
                                    int y0, int y1, unsigned flags, int max_aniso, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_ANISO_H */
