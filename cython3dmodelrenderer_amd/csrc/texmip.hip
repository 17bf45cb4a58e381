// texmip.hip — the mip chain of a texture and the trilinear texture pass over the winner plane
// (include/crender_mip.h states the arithmetic; this file keeps its operation order).
//
// The pass keeps texture.hip's shape: a pixel per work item, an 8 x 8 block of pixels per wavefront (a
// workgroup is four of them side by side: 32 x 8), and a wavefront whose 64 winners are all background,
// with no light to apply, leaves after its one load.  A covered pixel projects its winner once and takes
// the barycentrics of (x, y), (x + 1, y) and (x, y + 1): the nine edge constants and the reciprocals of the
// three denominators are the triangle's (raster_math.h's TriSetup), so the two neighbours cost their
// numerators and the short tails of their divisions.  The level comes from the exponent field of rho (no
// logarithm), and a lane whose weight f is zero — every magnified pixel — skips the second level's four
// texels: a magnified frame fetches what the bilinear pass fetches, and pays for two more uv evaluations
// (README, "Per-pixel texture mapping": T-Rex 4096^2 62 us against 53 us affine, 73 against 55 perspective,
// and parity under the fused light, where the planes' bytes set the time).
//
// The chain is built once per bound texture, a launch per level, each a 2 x 2 box over the level before.
#include "common.h"
#include "../../include/crender_mip.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, bilinear, store_shaded, pass_grid
#include "mip_sample.h"      // chain_layout, MipChain, mip_chain, mip_level, pixel_uv

namespace {

template <bool PERSPECTIVE, bool LIGHT>
__global__ __launch_bounds__(kThreads) void k_mip_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                         int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                         const float *__restrict__ uv,
                                                         const unsigned char *__restrict__ chain, MipChain M,
                                                         const float *__restrict__ nb, Light L,
                                                         float *__restrict__ cb, int W, int y0, int y1, int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!LIGHT && !wave_any(px.covered)) continue;
        float col[3] = {0.0f, 0.0f, 0.0f};
        if (px.covered) {
            const PixelUV at = pixel_uv<PERSPECTIVE>(P, tri, uv, px);
            const float tu = at.tu, tv = at.tv;
            const float ftw = (float)M.tw, fth = (float)M.th;
            const float dudx = (at.ux - tu) * ftw, dvdx = (at.vx - tv) * fth;
            const float dudy = (at.uy - tu) * ftw, dvdy = (at.vy - tv) * fth;
            const float rx = dudx * dudx + dvdx * dvdx;
            const float ry = dudy * dudy + dvdy * dvdy;
            const float r2 = (rx >= ry) ? rx : ry;
            const float rho = sqrtf(r2);
            int l0;
            float f;
            mip_level(rho, M.L, l0, f);
            const int hl = max(1, M.th >> l0), wl = max(1, M.tw >> l0);
            bilinear(chain + (l0 ? M.off[l0] : 0ull), hl, wl, tu, tv, col);      // (level 0 needs no look at the table)
            if (f != 0.0f) {         // (only between two levels: l0 + 1 <= L - 1)
                float up[3];
                bilinear(chain + M.off[l0 + 1], max(1, hl >> 1), max(1, wl >> 1), tu, tv, up);
                const float g = 1.0f - f;
#pragma unroll
                for (int j = 0; j < 3; ++j) col[j] = col[j] * g + up[j] * f;
            }
        }
        store_shaded<LIGHT>(px, col, nb, L, cb);
    }
}

// Level k from level k - 1 (h x w): a destination texel per work item, its edge-clamped 2 x 2 block in integers.
__global__ __launch_bounds__(kThreads) void k_mip_reduce(const unsigned char *__restrict__ src, int h, int w,
                                                          unsigned char *__restrict__ dst, int hk, int wk)
{
    const size_t n = (size_t)hk * (size_t)wk;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const int r = (int)(i / (size_t)wk), c = (int)(i - (size_t)r * (size_t)wk);
        const int r0 = min(2 * r, h - 1), r1 = min(2 * r + 1, h - 1);
        const int c0 = min(2 * c, w - 1), c1 = min(2 * c + 1, w - 1);
        const unsigned char *A = texel(src, r0, c0, w), *B = texel(src, r0, c1, w);
        const unsigned char *C = texel(src, r1, c0, w), *D = texel(src, r1, c1, w);
        unsigned char *o = dst + i * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = (unsigned char)(((int)A[j] + (int)B[j] + (int)C[j] + (int)D[j] + 2) >> 2);
    }
}

}  // namespace

extern "C" {

int crender_mip_layout(int th, int tw, int *levels, int *h16, int *w16, uint64_t *offset16, uint64_t *total_bytes)
{
    int L, h[kMaxLevels], w[kMaxLevels];
    unsigned long long off[kMaxLevels], total;
    if (!chain_layout(th, tw, L, h, w, off, total))
        return fail(CRENDER_EINVAL, "crender_mip_layout: a side below 1 or above 65535");
    if (levels) *levels = L;
    for (int k = 0; k < kMaxLevels; ++k) {
        if (h16) h16[k] = h[k];
        if (w16) w16[k] = w[k];
        if (offset16) offset16[k] = off[k];
    }
    if (total_bytes) *total_bytes = total;
    return CRENDER_OK;
}

int crender_mip_build(const unsigned char *d_texture, int th, int tw, unsigned char *d_chain, void *stream)
{
    int L, h[kMaxLevels], w[kMaxLevels];
    unsigned long long off[kMaxLevels], total;
    if (!d_texture || !d_chain || !chain_layout(th, tw, L, h, w, off, total))
        return fail(CRENDER_EINVAL, "crender_mip_build: bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CR_HIP(hipMemcpyAsync(d_chain, d_texture, 3 * (size_t)th * (size_t)tw, hipMemcpyDeviceToDevice, st));
    for (int k = 1; k < L; ++k) {
        const int grid = grid_for((size_t)h[k] * (size_t)w[k], 16384);
        hipLaunchKernelGGL(k_mip_reduce, dim3(grid), dim3(kThreads), 0, st, d_chain + off[k - 1], h[k - 1], w[k - 1],
                           d_chain + off[k], h[k], w[k]);
        CR_LAUNCH_CHECK("k_mip_reduce");
    }
    return CRENDER_OK;
}

int crender_mip_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                      const float *P16, const float *d_uv, const unsigned char *d_chain, int th, int tw,
                      const float *d_normal, const float *light3, float *d_color, int H, int W, int y0, int y1,
                      unsigned flags, void *stream)
{
    MipChain M;
    if (!frame_args_ok(d_winner, P16, d_color, T, d_tri, H, W, y0, y1) || !d_chain || (T > 0 && !d_uv) ||
        !mip_chain(th, tw, M) || !light_args_ok(light3, d_normal) || (flags & ~(unsigned)CRENDER_MIP_PERSPECTIVE))
        return fail(CRENDER_EINVAL, "crender_mip_shade: bad argument");
    const bool light = light3 != nullptr;
    if (T == 0 && !light) return CRENDER_OK;
    const bool persp = flags & CRENDER_MIP_PERSPECTIVE;
    // [perspective][light]
    static constexpr decltype(&k_mip_shade<false, false>) kernels[2][2] = {
        {k_mip_shade<false, false>, k_mip_shade<false, true>}, {k_mip_shade<true, false>, k_mip_shade<true, true>}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[persp][light], G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner,
                       d_tri, T, d_pos_of, make_proj(P16, W, H), d_uv, d_chain, M, d_normal, pass_light(light3),
                       d_color, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_mip_shade");
    return CRENDER_OK;
}

}  // extern "C"
