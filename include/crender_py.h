/*
 * crender_py.h — C ABI of the numpy filler (crender/py's AdvancedPixelBufferFiller) of
 * libcrender_hip.so.  Same conventions as crender_hip.h and crender_wire.h: raw device pointers, an
 * int status (CRENDER_OK or a CRENDER_E* code, text in crender_last_error()), work enqueued on
 * `stream` and nothing synchronised.  Reference files cited below are in the reference's crender/py/.
 *
 * Result contract: after crender_py_draw the three planes hold, bit for bit, what
 * AdvancedPixelBufferFiller.compute_triangle_statistics (pixel_buffer_filler/
 * advanced_pixel_buffer_filler.py:39-240) leaves when the py Renderer (renderer.py:52-59) calls it on
 * triangle 0, 1, ..., T-1 of the given (already ordered) arrays, on numpy 2.2 with OpenBLAS 0.3.29.
 * Per triangle, "fma" a single rounding, l0 l1 l2 the barycentrics of a pixel:
 *   1. cull (:59, :66): the float32 2-D cross a0*b1 - a1*b0 of the raw (v1-v0).xy, (v2-v0).xy is 0; or
 *      the float32 mean normal m = ((n0+n1)+n2) / 3 has finite x and y and m.z >= 0 (the float64 dot
 *      of [0,0,1] with it; an inf or NaN in x / y makes it NaN: not culled; a z sum of -2^-149 gives
 *      m.z = -0: culled);
 *   2. project (:84-105), float32: x*P00, y*P11, (z*P22) + P32 (two roundings), each divided by the
 *      raw z, x and y then +1 and times W/2, H/2 (the P's are numpy's float32 projection matrix);
 *   3. box (:130-145): ceil of the float32 min / max, to int32 as x86 does (NaN or out of range ->
 *      INT_MIN), x clipped to [0, W], y to [0, H]; pixels x in [xl, xr), y in [ceil min y, ceil max y);
 *   4. barycentrics (:176-178): l0 = ((x1-x2)*(y-y2) - (y1-y2)*(x-x2)) / D0 with float32 differences
 *      of vertices, float64 pixel differences and products, D0 the float32 expression of the
 *      vertices, a correctly rounded float64 quotient (l1, l2 likewise); inside iff all are >= 0;
 *   5. depth (:224, BLAS dgemv / ddot): n = number of inside pixels of the triangle;
 *      z = fma(l2, z2, fma(l0, z0, l1*z1)) for n >= 2, fma(l2, z2, fma(l1, z1, l0*z0)) for n = 1;
 *   6. a pixel is written iff 0 <= z <= 1 and z < (double)stored_z (:227-238); z stores as float32;
 *   7. attributes (:189-206): v = fma(l2, v2, fma(l1, v1, l0*v0)) in float64 per component; normals
 *      store as float32, colours as numpy's float64 -> uint8 cast on x86 (truncation to int32, NaN or
 *      out of range -> INT_MIN, low byte).
 * The sequential rule of 6 is resolved in one pass with a uint64 atomicMin per pixel: key =
 * (ordered bits of float32(z), class, tiebreak), class 0 with tiebreak 2^31-1-rank for z < float32(z),
 * class 1 with tiebreak rank otherwise, rank = triangle + 1; the plane's current z seeds rank 0.
 *
 * Domain: T < 2^30, 1 <= H, W <= 2^15, and every vertex coordinate, normal and colour component finite
 * with vertex z != 0 (z = +-0 makes the sign of the perspective divide depend on BLAS's summation order).
 * Outside it *d_status is set to 1 and the call draws NOTHING: the planes keep their contents,
 * CRENDER_PY_CLEAR included.  *d_status is 0 otherwise.
 */
#ifndef CRENDER_PY_H
#define CRENDER_PY_H

#include "crender_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of crender_py_draw */
enum {
    CRENDER_PY_CLEAR = 1u            /* first set z = 1e6, colour = normal = 0 (the py Renderer's initial
                                      * buffers), under the same domain check */
};

/* Bytes of the scratch crender_py_draw needs for T triangles on an H x W frame: the uint64 key plane
 * [H][W], 76 bytes per triangle and 8 per 256 triangles, each part rounded up to 16 bytes.  Its
 * contents need no initial value.  0 for a bad size. */
CRENDER_API size_t crender_py_scratch_bytes(int H, int W, int64_t T);

/* Draw T triangles, in array order, onto the planes.
 *   d_tri, d_col, d_nrm  float32 [T][3][3]: vertices, colours (BGR per corner), vertex normals
 *   proj4                HOST float[4]: P00, P11, P22, P32 of the filler's float32 projection matrix
 *   d_z       float32 [H][W]       (Renderer.z_buffer)
 *   d_color   uint8   [H][W][3]    (Renderer.color_buffer)
 *   d_normal  float32 [H][W][3]    (Renderer.n_buffer)
 *   d_scratch crender_py_scratch_bytes(H, W, T) bytes, 16-byte aligned (else CRENDER_EINVAL)
 *   d_status  DEVICE int32 [1]: 0, or 1 if an input is out of the domain (nothing drawn)
 * Up to seven launches; no synchronisation.  The pixels of every box are spread over a fixed grid, so a
 * triangle covering much of the frame is drawn by every CU. */
CRENDER_API int crender_py_draw(const float *d_tri, const float *d_col, const float *d_nrm, int64_t T,
                                const float *proj4, float *d_z, uint8_t *d_color, float *d_normal, int H, int W,
                                unsigned flags, void *d_scratch, int32_t *d_status, void *stream);

/* The py GuroIllumination (illumination/guro_illumination.py:20-27) on the uint8 colour plane:
 * c = clip(s / (m + 1e-6f), 0, 1) with s = ((0 + n0*l0) + n1*l1) + n2*l2, m = sqrt((n0*n0 + n1*n1) +
 * n2*n2) in float32, then colour = uint8(float32(colour) * c) (truncation; NaN -> 0).  light3: HOST
 * float[3], the illumination's normalised, negated light direction. */
CRENDER_API int crender_py_guro(uint8_t *d_color, const float *d_normal, const float *light3, int H, int W,
                                void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CRENDER_PY_H */
