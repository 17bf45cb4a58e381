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

#include "mip_sample.h"      // chain_layout, MipChain, bilinear, CornerUV, uv_at

namespace {

template <bool PERSPECTIVE, bool LIGHT>
__global__ __launch_bounds__(kThreads) void k_mip_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                         int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                         const float *__restrict__ uv,
                                                         const unsigned char *__restrict__ chain, MipChain M,
                                                         const float *__restrict__ nb, Light L,
                                                         float *__restrict__ cb, int W, int y0, int y1, int row_blocks)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = ((int)blockIdx.x * (kThreads / 64) + wave) * kTexBlock + (lane & (kTexBlock - 1));
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const int y = y0 + rb * kTexBlock + (lane >> 3);
        const bool inside = x < W && y < y1;
        const size_t pix = (size_t)y * (size_t)W + (size_t)x;
        int64_t orig = -1;           // the winner in the caller's order (uv), and where it sits in d_tri
        if (inside) orig = win[pix];
        bool covered = orig >= 0 && orig < T;
        int64_t t = orig;
        if (covered && pos_of) {
            t = pos_of[orig];
            covered = t < T;
        }
        if (!LIGHT && !wave_any(covered)) continue;
        float col[3] = {0.0f, 0.0f, 0.0f};
        if (covered) {
            float a[3], b[3], c[3];
            const float *v = tri + t * 9;
            a[0] = v[0]; a[1] = v[1]; a[2] = v[2];
            b[0] = v[3]; b[1] = v[4]; b[2] = v[5];
            c[0] = v[6]; c[1] = v[7]; c[2] = v[8];
            const float *w = uv + orig * 6;
            CornerUV K{w[0], w[1], w[2], w[3], w[4], w[5], a[2], b[2], c[2], 0.0f, 0.0f, 0.0f, false};
            if (PERSPECTIVE && in_div_window(K.za) && in_div_window(K.zb) && in_div_window(K.zc)) {
                K.ra = refined_rcp(K.za); K.rb = refined_rcp(K.zb); K.rc = refined_rcp(K.zc);
                K.z_fast = true;
            }
            project_vertex(P, a);
            project_vertex(P, b);
            project_vertex(P, c);
            const TriSetup S = make_setup(TriXYZ{a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]}, true);
            float tu, tv, ux, vx, uy, vy;
            uv_at<PERSPECTIVE>(S, K, x, y, tu, tv);
            uv_at<PERSPECTIVE>(S, K, x + 1, y, ux, vx);
            uv_at<PERSPECTIVE>(S, K, x, y + 1, uy, vy);
            const float ftw = (float)M.tw, fth = (float)M.th;
            const float dudx = (ux - tu) * ftw, dvdx = (vx - tv) * fth;
            const float dudy = (uy - tu) * ftw, dvdy = (vy - tv) * fth;
            const float rx = dudx * dudx + dvdx * dvdx;
            const float ry = dudy * dudy + dvdy * dvdy;
            const float r2 = (rx >= ry) ? rx : ry;
            const float rho = sqrtf(r2);
            int l0 = 0;
            float f = 0.0f;
            if (rho > 1.0f) {
                if (!(rho < (float)(1u << (M.L - 1)))) {
                    l0 = M.L - 1;
                } else {
                    // 1 < rho < 2^15: a normal number whose exponent field is the level, and whose
                    // significand, scaled back by the exact power of two, is 1 + f
                    l0 = (int)(__float_as_uint(rho) >> 23) - 127;
                    f = rho * __uint_as_float((uint32_t)(127 - l0) << 23) - 1.0f;
                }
            }
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
        if (LIGHT) {
            if (!inside) continue;
            float *cp = cb + pix * 3;
            const float *np_ = nb + pix * 3;
            if (!covered) { col[0] = cp[0]; col[1] = cp[1]; col[2] = cp[2]; }
            const float s = guro_factor(L, np_[0], np_[1], np_[2]);
            cp[0] = col[0] * s; cp[1] = col[1] * s; cp[2] = col[2] * s;
        } else if (covered) {
            float *cp = cb + pix * 3;
            cp[0] = col[0]; cp[1] = col[1]; cp[2] = col[2];
        }
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

template <bool PERSPECTIVE>
void launch_mip(bool light, dim3 grid, hipStream_t st, const int32_t *win, const float *tri, int64_t T,
                const uint32_t *pos_of, const ProjConst &P, const float *uv, const unsigned char *chain,
                const MipChain &M, const float *nb, const Light &L, float *cb, int W, int y0, int y1, int row_blocks)
{
    if (light)
        hipLaunchKernelGGL((k_mip_shade<PERSPECTIVE, true>), grid, dim3(kThreads), 0, st, win, tri, T, pos_of, P, uv,
                           chain, M, nb, L, cb, W, y0, y1, row_blocks);
    else
        hipLaunchKernelGGL((k_mip_shade<PERSPECTIVE, false>), grid, dim3(kThreads), 0, st, win, tri, T, pos_of, P, uv,
                           chain, M, nb, L, cb, W, y0, y1, row_blocks);
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
    int h[kMaxLevels], w[kMaxLevels];
    unsigned long long total;
    if (!d_winner || !P16 || !d_chain || !d_color || T < 0 || (T > 0 && (!d_tri || !d_uv)) ||
        !chain_layout(th, tw, M.L, h, w, M.off, total) || H < 1 || W < 1 || y0 < 0 || y1 > H || y0 >= y1 ||
        (light3 && !d_normal) || (d_normal && !light3) || (flags & ~(unsigned)CRENDER_MIP_PERSPECTIVE))
        return fail(CRENDER_EINVAL, "crender_mip_shade: bad argument");
    M.th = th;
    M.tw = tw;
    const bool light = light3 != nullptr;
    if (T == 0 && !light) return CRENDER_OK;
    const ProjConst P = make_proj(P16, W, H);
    const Light L = light ? Light{light3[0], light3[1], light3[2], 1} : Light{0.0f, 0.0f, 0.0f, 0};
    const int row_blocks = (y1 - y0 + kTexBlock - 1) / kTexBlock;
    const int across = kTexBlock * (kThreads / 64);
    const dim3 grid((unsigned)((W + across - 1) / across), (unsigned)(row_blocks < 65535 ? row_blocks : 65535));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags & CRENDER_MIP_PERSPECTIVE)
        launch_mip<true>(light, grid, st, d_winner, d_tri, T, d_pos_of, P, d_uv, d_chain, M, d_normal, L, d_color, W,
                         y0, y1, row_blocks);
    else
        launch_mip<false>(light, grid, st, d_winner, d_tri, T, d_pos_of, P, d_uv, d_chain, M, d_normal, L, d_color, W,
                          y0, y1, row_blocks);
    CR_LAUNCH_CHECK("k_mip_shade");
    return CRENDER_OK;
}

}  // extern "C"
