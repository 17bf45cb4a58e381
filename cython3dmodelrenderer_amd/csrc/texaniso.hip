// texaniso.hip — the anisotropic texture pass over the winner plane (include/crender_aniso.h states the
// arithmetic; this file keeps its operation order).
//
// k_mip_shade's shape (texmip.hip): a pixel per work item, an 8 x 8 block of pixels per wavefront, a wavefront
// with no covered pixel and no light leaves after its winner load, and the three uv evaluations of a pixel share
// one TriSetup.  New per covered lane: the second square root, two divisions, and N trilinear samples along the
// major axis, summed in three registers.  Everything a sample needs per level — the two pointers, heights and
// widths, f and 1 - f — is formed before the loop (the (float) forms of the sizes inside bilinear() are loop
// invariants the compiler hoists with them).
//
// The sample loop is ONE loop for every lane, each lane leaving after its own N iterations: a lane with N == 1
// samples (u, v) itself — its offset is never formed into the coordinates, as the contract asks — and skips the
// final division.  The trip count is left to diverge: the compiler masks a lane off once its own N is reached
// and the wavefront runs to its largest.  The other form — the wavefront's largest N found first (wave_reduce)
// and every covered lane driven through that many iterations, a finished lane sampling (u, v) again and its
// result dropped by a select — gave the same bits and was slower on 43 of 48 rows of scripts/tex_time.py,
// by 1 to 7 % where lanes mix sample counts (T-Rex 1024^2, A = 4: 15.2 against 16.2 us; 4096^2 perspective:
// 85.8 against 88.4 us): a finished lane's fetches are not free, and its state stays live across the reduction.
// It won only where every lane runs the same N anyway (the floor, affine, A = 16: 24.3 against 25.9 us).
#include "common.h"
#include "../../include/crender_aniso.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, bilinear, store_shaded, pass_grid
#include "mip_sample.h"      // MipChain, mip_chain, mip_level, pixel_uv

namespace {

template <bool PERSPECTIVE, bool LIGHT>
__global__ __launch_bounds__(kThreads) void k_aniso_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                           int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                           const float *__restrict__ uv,
                                                           const unsigned char *__restrict__ chain, MipChain M,
                                                           const float *__restrict__ nb, Light L,
                                                           float *__restrict__ cb, int W, int y0, int y1, int row_blocks,
                                                           int A)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!LIGHT && !wave_any(px.covered)) continue;
        float col[3] = {0.0f, 0.0f, 0.0f};
        if (px.covered) {
            const PixelUV at = pixel_uv<PERSPECTIVE>(P, tri, uv, px);
            const float tu = at.tu, tv = at.tv;
            const float ftw = (float)M.tw, fth = (float)M.th;
            const float dux = at.ux - tu, dvx = at.vx - tv, duy = at.uy - tu, dvy = at.vy - tv;
            const float dudx = dux * ftw, dvdx = dvx * fth;
            const float dudy = duy * ftw, dvdy = dvy * fth;
            const float rx = dudx * dudx + dvdx * dvdx;
            const float ry = dudy * dudy + dvdy * dvdy;
            const bool x_major = rx >= ry;
            const float pmax = sqrtf(x_major ? rx : ry), pmin = sqrtf(x_major ? ry : rx);
            const float du = x_major ? dux : duy, dv = x_major ? dvx : dvy;
            // the level from the minor axis, widened to pmax / A and to one texel; N samples span the major one
            float rho = pmax;
            int N = 1;
            if (pmax > 1.0f) {
                const float fa = (float)A;
                const float lo = pmax / fa;
                rho = (pmin >= lo) ? pmin : lo;
                rho = (rho >= 1.0f) ? rho : 1.0f;
                const float q = pmax / rho;
                if (q > 1.0f) {
                    const float nf = ceilf(q);
                    N = (nf < fa) ? (int)nf : A;
                }
            }
            int l0;
            float f;
            mip_level(rho, M.L, l0, f);
            const int hl = max(1, M.th >> l0), wl = max(1, M.tw >> l0);
            const unsigned char *lower = chain + (l0 ? M.off[l0] : 0ull);       // (level 0 needs no look at the table)
            const bool two = f != 0.0f;      // (only between two levels: l0 + 1 <= L - 1)
            const unsigned char *upper = two ? chain + M.off[l0 + 1] : lower;
            const int hu = max(1, hl >> 1), wu = max(1, wl >> 1);
            const float g = 1.0f - f;
            const float fn = (float)N, den = (float)(2 * N);
            for (int i = 0; i < N; ++i) {
                float su = tu, sv = tv;
                if (N > 1) {
                    const float o = (float)(2 * i + 1 - N) / den;
                    su = tu + du * o;
                    sv = tv + dv * o;
                }
                float ci[3];
                bilinear(lower, hl, wl, su, sv, ci);
                if (two) {
                    float up[3];
                    bilinear(upper, hu, wu, su, sv, up);
#pragma unroll
                    for (int j = 0; j < 3; ++j) ci[j] = ci[j] * g + up[j] * f;
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) col[j] = i ? col[j] + ci[j] : ci[j];
            }
            if (N > 1) {
#pragma unroll
                for (int j = 0; j < 3; ++j) col[j] = col[j] / fn;
            }
        }
        store_shaded<LIGHT>(px, col, nb, L, cb);
    }
}

}  // namespace

extern "C" {

int crender_aniso_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                        const float *P16, const float *d_uv, const unsigned char *d_chain, int th, int tw,
                        const float *d_normal, const float *light3, float *d_color, int H, int W, int y0, int y1,
                        unsigned flags, int max_aniso, void *stream)
{
    MipChain M;
    if (!frame_args_ok(d_winner, P16, d_color, T, d_tri, H, W, y0, y1) || !d_chain || (T > 0 && !d_uv) ||
        !mip_chain(th, tw, M) || !light_args_ok(light3, d_normal) || (flags & ~(unsigned)CRENDER_MIP_PERSPECTIVE) ||
        max_aniso < 1 || max_aniso > CRENDER_ANISO_MAX)
        return fail(CRENDER_EINVAL, "crender_aniso_shade: bad argument");
    const bool light = light3 != nullptr;
    if (T == 0 && !light) return CRENDER_OK;
    const bool persp = flags & CRENDER_MIP_PERSPECTIVE;
    // [perspective][light]
    static constexpr decltype(&k_aniso_shade<false, false>) kernels[2][2] = {
        {k_aniso_shade<false, false>, k_aniso_shade<false, true>}, {k_aniso_shade<true, false>, k_aniso_shade<true, true>}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[persp][light], G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner,
                       d_tri, T, d_pos_of, make_proj(P16, W, H), d_uv, d_chain, M, d_normal, pass_light(light3),
                       d_color, W, y0, y1, G.row_blocks, max_aniso);
    CR_LAUNCH_CHECK("k_aniso_shade");
    return CRENDER_OK;
}

}  // extern "C"
