// peel.hip — transparency: depth peeling by depth key and the blend of a layer under what is in front of it
// (include/crender_peel.h states the arithmetic; this file keeps its operation order).
#include <math.h>

#include "common.h"
#include "../../include/crender_peel.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, winner_triangle, pass_grid, frame_checks

// ---- transparency (crender_peel_next, crender_peel_blend) ----
// Depth peeling by depth key.  A frame leaves the two halves of every pixel's winning key behind, the z plane and the
// winner plane; the layer behind it is, per pixel, the fragment with the LEAST key strictly above that one: no epsilon,
// coplanar duplicates peel one by one, and being a minimum of unique 64-bit keys it comes out bit for bit whatever the
// launch order.  crender_peel_next is crender_raster_atomic's walk (raster.hip: k_keys_init, k_cover_atomic,
// k_resolve_global) with one more test per sample, three launches:
//   k_peel_seed     a pixel per work item: the key plane gets the cleared key where the previous layer is valid (its
//                   winner is a triangle, its z is not NaN) and 0 where it is not — no key is below 0, so an exhausted
//                   pixel never takes a fragment and the cover pass needs no validity test of its own.
//   k_peel_cover    a wavefront per triangle of the caller's order (through pos_of to where it lies in d_tri), 8 x 8
//                   pixels per step over the pixel box clipped to the rows.  Per sample: the barycentrics (three correctly
//                   rounded divisions) and z, as every coverage pass pays them; for a sample that is a fragment 16 bytes
//                   of plain loads — the slot's key, then the previous winner and z, from which K is rebuilt — and the
//                   64-bit atomicMin only if K < k and k < *slot (the slot only ever falls, so a stale read costs an
//                   atomic, never a result).  A wavefront owns its triangle's WHOLE box: one frame-sized triangle is
//                   (W / 8) (H / 8) serial steps of one wavefront (1 024 at 256^2, 262 144 at 4096^2) while the rest of
//                   the device idles; boxes are not split among wavefronts.  The grid is capped at kPeelMaxGrid
//                   workgroups, 4 wavefronts each: beyond 32 768 triangles a wavefront takes further trips.
//   k_peel_resolve  a pixel per work item: the slot's low word names the fragment, whose z is computed again by the same
//                   device functions — the very value the key was built from, a -0 as -0 — and stored with the index;
//                   a slot still at its seed stores winner -1 and z 1e6f.
// crender_peel_blend puts one layer under what is in front of it, a per-pixel pass of the shape of k_env_shade: a pixel
// per lane, no LDS, 4 bytes of winner a pixel and for a pixel that blends its transmittance, alpha, the winner's 27
// floats of corners, colours and normals (or 12 bytes of the front plane), three divisions, and 16 bytes stored.

namespace {

constexpr int kPeelMaxGrid = 8192;           // workgroups of the cover launch: 32 768 wavefronts; the kernel loops

// Whether the previous layer's pixel names a fragment, and then its key.
__device__ inline bool peel_prev_key(int32_t w, float z, int64_t T, const uint32_t *__restrict__ pos_of,
                                     unsigned long long &K)
{
    if (w < 0 || (int64_t)w >= T || z != z) return false;
    if (pos_of && (int64_t)pos_of[w] >= T) return false;
    K = fragment_key(z, (uint32_t)w);
    return true;
}

__global__ __launch_bounds__(kThreads) void k_peel_seed(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                         int64_t T, const uint32_t *__restrict__ pos_of,
                                                         unsigned long long *__restrict__ keys, size_t first_pix,
                                                         size_t npix)
{
    const size_t stride = (size_t)gridDim.x * kThreads;
    const unsigned long long key_clear = make_key(zord(1e6f), KEY_LOW_PRIOR);
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += stride) {
        const size_t pix = first_pix + i;
        unsigned long long K;
        keys[pix] = peel_prev_key(win[pix], zb[pix], T, pos_of, K) ? key_clear : 0ull;
    }
}

__global__ __launch_bounds__(kThreads) void k_peel_cover(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                          const float *__restrict__ tri, const float *__restrict__ nrm,
                                                          int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                          unsigned long long *__restrict__ keys, int W, int H, int y0,
                                                          int y1)
{
    const int l = threadIdx.x & 63, lx = l & 7, ly = l >> 3;
    const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * kThreads) >> 6;
    for (int64_t i = wave; i < T; i += nwaves) {             // i: the caller's index, the winner plane's word
        const int64_t t = pos_of ? (int64_t)pos_of[i] : i;
        if (t >= T) continue;
        const float *nn = nrm + t * 9;
        if (backface(nn[2], nn[5], nn[8])) continue;
        const TriXYZ tr = winner_triangle(tri, t, P);
        int xl, xr, yt, yb;
        pixel_box(tr.x0, tr.y0, tr.x1, tr.y1, tr.x2, tr.y2, W, H, xl, xr, yt, yb);
        if (xl - xr == 0 || yt - yb == 0) continue;
        if (yt < y0) yt = y0;
        if (yb > y1) yb = y1;
        for (int yy = yt + ly; yy < yb; yy += 8)
            for (int xx = xl + lx; xx < xr; xx += 8) {
                unsigned long long k;
                if (!fragment(tr, (uint32_t)i, xx, yy, k)) continue;
                const size_t pix = (size_t)yy * (size_t)W + (size_t)xx;
                unsigned long long *slot = &keys[pix];
                if (!(k < *slot)) continue;                  // (0 where the previous layer is not valid)
                const unsigned long long K = fragment_key(zb[pix], (uint32_t)win[pix]);
                if (K < k) atomicMin(slot, k);
            }
    }
}

__global__ __launch_bounds__(kThreads) void k_peel_resolve(const float *__restrict__ tri,
                                                            const uint32_t *__restrict__ pos_of, ProjConst P,
                                                            const unsigned long long *__restrict__ keys,
                                                            int32_t *__restrict__ win_out, float *__restrict__ z_out, int W,
                                                            size_t first_pix, size_t npix)
{
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += stride) {
        const size_t pix = first_pix + i;
        const unsigned long long key = keys[pix];
        const uint32_t low = (uint32_t)key;
        int32_t w = -1;
        float z = 1e6f;
        if (key != 0ull && low != KEY_LOW_PRIOR) {
            const uint32_t id = 0xFFFFFFFEu - low;
            const int64_t t = pos_of ? (int64_t)pos_of[id] : (int64_t)id;
            const TriXYZ tr = winner_triangle(tri, t, P);
            float b1, b2, b3;
            barycentric(tr, (int)(pix % (size_t)W), (int)(pix / (size_t)W), b1, b2, b3);
            z = interp(tr.z0, tr.z1, tr.z2, b1, b2, b3);
            w = (int32_t)id;
        }
        win_out[pix] = w;
        z_out[pix] = z;
    }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kThreads) void k_peel_blend(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                          int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                          const float *__restrict__ col, const float *__restrict__ nrm,
                                                          const float *__restrict__ alpha, Light L,
                                                          const float *__restrict__ front, float bg0, float bg1, float bg2,
                                                          float *__restrict__ trans, float *__restrict__ ob, int W, int y0,
                                                          int y1, int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!FIRST && !LAST && !wave_any(px.covered)) continue;     // a scalar branch: the whole wavefront leaves
        if (!px.inside) continue;
        float *op = ob + px.pix * 3;
        float t = FIRST ? 1.0f : trans[px.pix];
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
        bool wrote = false;
        if (px.covered && t > 0.0f) {
            float a = alpha[px.orig];
            a = a > 0.0f ? a : 0.0f;                                 // (a NaN gives 0)
            a = a > 1.0f ? 1.0f : a;
            float c0, c1, c2;
            if (FIRST && front) {
                const float *fp = front + px.pix * 3;
                c0 = fp[0]; c1 = fp[1]; c2 = fp[2];
            } else {
                const TriXYZ X = winner_triangle(tri, px.t, P);
                float c[9], n[9], b1, b2, b3;
                load9(col + px.t * 9, c);
                load9(nrm + px.t * 9, n);
                barycentric(X, px.x, px.y, b1, b2, b3);
                const Shade s = shade_fragment(c, n, b1, b2, b3, L);
                c0 = s.c0; c1 = s.c1; c2 = s.c2;
            }
            const float g = t * a;
            if (FIRST) {
                o0 = g * c0; o1 = g * c1; o2 = g * c2;
            } else {
                o0 = op[0] + g * c0; o1 = op[1] + g * c1; o2 = op[2] + g * c2;
            }
            t = t * (1.0f - a);
            wrote = true;
        } else if (FIRST) {
            wrote = true;                                            // no triangle: out = 0, trans = 1
        }
        if (LAST && t > 0.0f) {
            if (!wrote) { o0 = op[0]; o1 = op[1]; o2 = op[2]; }
            o0 = o0 + t * bg0; o1 = o1 + t * bg1; o2 = o2 + t * bg2;
            op[0] = o0; op[1] = o1; op[2] = o2;
            if (wrote) trans[px.pix] = t;
        } else if (wrote) {
            op[0] = o0; op[1] = o1; op[2] = o2;
            trans[px.pix] = t;
        }
    }
}

}  // namespace

extern "C" {

int crender_peel_next(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                      const float *P16, const float *d_nrm, void *d_keys, int32_t *d_winner_out, float *d_z_out, int H,
                      int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_peel_next";
    if (!d_winner || !d_z || !P16 || !d_keys || !d_winner_out || !d_z_out)
        return arg_error(E, "d_winner, d_z, P16, d_keys, d_winner_out or d_z_out is NULL");
    if (int rc = frame_checks(E, T, d_tri && d_nrm, H, W, "d_tri or d_nrm is NULL with T > 0")) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags) return arg_error(E, "unknown flag bits");
    if (T > 0x7FFFFFFFll) return arg_error(E, "T is above 2^31 - 1 (the winner plane is int32)");
    if (d_winner_out == d_winner || d_z_out == d_z) return arg_error(E, "an output plane is its input (the peel cannot run in place)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t first = (size_t)y0 * (size_t)W, npix = (size_t)(y1 - y0) * (size_t)W;
    unsigned long long *keys = static_cast<unsigned long long *>(d_keys);
    const ProjConst P = make_proj(P16, W, H);
    hipLaunchKernelGGL(k_peel_seed, dim3(grid_for(npix, 4096)), dim3(kThreads), 0, s, d_winner, d_z, T, d_pos_of, keys, first,
                       npix);
    CR_LAUNCH_CHECK("k_peel_seed");
    if (T > 0) {
        hipLaunchKernelGGL(k_peel_cover, dim3(grid_for((size_t)T * 64, kPeelMaxGrid)), dim3(kThreads), 0, s, d_winner, d_z,
                           d_tri, d_nrm, T, d_pos_of, P, keys, W, H, y0, y1);
        CR_LAUNCH_CHECK("k_peel_cover");
    }
    hipLaunchKernelGGL(k_peel_resolve, dim3(grid_for(npix, 8192)), dim3(kThreads), 0, s, d_tri, d_pos_of, P, keys,
                       d_winner_out, d_z_out, W, first, npix);
    CR_LAUNCH_CHECK("k_peel_resolve");
    return CRENDER_OK;
}

int crender_peel_blend(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of, const float *P16,
                       const float *d_col, const float *d_nrm, const float *d_alpha, const float *light3,
                       const float *d_front, const float *background3, float *d_trans, float *d_out, int H, int W, int y0,
                       int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_peel_blend";
    const bool first = flags & CRENDER_PEEL_FIRST, last = flags & CRENDER_PEEL_LAST;
    if (!d_winner || !P16 || !background3 || !d_trans || !d_out)
        return arg_error(E, "d_winner, P16, background3, d_trans or d_out is NULL");
    if (int rc = frame_checks(E, T, d_tri && d_col && d_nrm && d_alpha, H, W, "d_tri, d_col, d_nrm or d_alpha is NULL with T > 0"))
        return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags & ~(unsigned)(CRENDER_PEEL_FIRST | CRENDER_PEEL_LAST)) return arg_error(E, "unknown flag bits");
    if (d_front && !first) return arg_error(E, "d_front is given without CRENDER_PEEL_FIRST");
    if (d_front == d_out) return arg_error(E, "d_out is d_front (the blend cannot run in place)");
    if (!(isfinite(background3[0]) && isfinite(background3[1]) && isfinite(background3[2])))
        return arg_error(E, "background3 is not finite");
    if (light3 && !(isfinite(light3[0]) && isfinite(light3[1]) && isfinite(light3[2])))
        return arg_error(E, "light3 is not finite");
    const ProjConst P = make_proj(P16, W, H);
    static constexpr decltype(&k_peel_blend<false, false>) kernels[2][2] = {
        {k_peel_blend<false, false>, k_peel_blend<false, true>}, {k_peel_blend<true, false>, k_peel_blend<true, true>}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[first][last], G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner, d_tri, T,
                       d_pos_of, P, d_col, d_nrm, d_alpha, pass_light(light3), d_front, background3[0], background3[1],
                       background3[2], d_trans, d_out, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_peel_blend");
    return CRENDER_OK;
}

}  // extern "C"
