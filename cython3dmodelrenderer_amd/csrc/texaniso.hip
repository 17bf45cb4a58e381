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

#include "mip_sample.h"      // chain_layout, MipChain, bilinear, CornerUV, uv_at

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
            const float dux = ux - tu, dvx = vx - tv, duy = uy - tu, dvy = vy - tv;
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
            int l0 = 0;
            float f = 0.0f;
            if (rho > 1.0f) {
                if (!(rho < (float)(1u << (M.L - 1)))) {
                    l0 = M.L - 1;
                } else {
                    // 1 < rho < 2^15: the exponent field is the level, the scaled significand is 1 + f (texmip.hip)
                    l0 = (int)(__float_as_uint(rho) >> 23) - 127;
                    f = rho * __uint_as_float((uint32_t)(127 - l0) << 23) - 1.0f;
                }
            }
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

template <bool PERSPECTIVE>
void launch_aniso(bool light, dim3 grid, hipStream_t st, const int32_t *win, const float *tri, int64_t T,
                  const uint32_t *pos_of, const ProjConst &P, const float *uv, const unsigned char *chain,
                  const MipChain &M, const float *nb, const Light &L, float *cb, int W, int y0, int y1, int row_blocks,
                  int A)
{
    if (light)
        hipLaunchKernelGGL((k_aniso_shade<PERSPECTIVE, true>), grid, dim3(kThreads), 0, st, win, tri, T, pos_of, P, uv,
                           chain, M, nb, L, cb, W, y0, y1, row_blocks, A);
    else
        hipLaunchKernelGGL((k_aniso_shade<PERSPECTIVE, false>), grid, dim3(kThreads), 0, st, win, tri, T, pos_of, P, uv,
                           chain, M, nb, L, cb, W, y0, y1, row_blocks, A);
}

}  // namespace

extern "C" {

int crender_aniso_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                        const float *P16, const float *d_uv, const unsigned char *d_chain, int th, int tw,
                        const float *d_normal, const float *light3, float *d_color, int H, int W, int y0, int y1,
                        unsigned flags, int max_aniso, void *stream)
{
    MipChain M;
    int h[kMaxLevels], w[kMaxLevels];
    unsigned long long total;
    if (!d_winner || !P16 || !d_chain || !d_color || T < 0 || (T > 0 && (!d_tri || !d_uv)) ||
        !chain_layout(th, tw, M.L, h, w, M.off, total) || H < 1 || W < 1 || y0 < 0 || y1 > H || y0 >= y1 ||
        (light3 && !d_normal) || (d_normal && !light3) || (flags & ~(unsigned)CRENDER_MIP_PERSPECTIVE) ||
        max_aniso < 1 || max_aniso > CRENDER_ANISO_MAX)
        return fail(CRENDER_EINVAL, "crender_aniso_shade: bad argument");
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
        launch_aniso<true>(light, grid, st, d_winner, d_tri, T, d_pos_of, P, d_uv, d_chain, M, d_normal, L, d_color, W,
                           y0, y1, row_blocks, max_aniso);
    else
        launch_aniso<false>(light, grid, st, d_winner, d_tri, T, d_pos_of, P, d_uv, d_chain, M, d_normal, L, d_color, W,
                            y0, y1, row_blocks, max_aniso);
    CR_LAUNCH_CHECK("k_aniso_shade");
    return CRENDER_OK;
}

}  // extern "C"
