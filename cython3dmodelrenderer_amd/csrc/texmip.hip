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

namespace {

constexpr int kTexBlock = 8;         // pixels along each side of a wavefront's block
constexpr int kMaxLevels = CRENDER_MIP_MAX_LEVELS;

// Where each level starts in the chain, by value in the kernel's arguments; a level's height and width are
// shifts of the texture's (h_k = max(1, th >> k)).
struct MipChain {
    unsigned long long off[kMaxLevels];
    int th, tw, L;
};

// The chain's shape; false for a texture crender_mip_layout refuses.
bool chain_layout(int th, int tw, int &L, int h[kMaxLevels], int w[kMaxLevels], unsigned long long off[kMaxLevels],
                  unsigned long long &total)
{
    if (th < 1 || tw < 1 || th > 65535 || tw > 65535) return false;
    const int side = th > tw ? th : tw;
    L = 0;
    while ((side >> L) > 0) ++L;     // 1 + floor(log2(side))
    total = 0;
    for (int k = 0; k < kMaxLevels; ++k) {
        const bool in = k < L;
        h[k] = in ? ((th >> k) > 1 ? (th >> k) : 1) : 0;
        w[k] = in ? ((tw >> k) > 1 ? (tw >> k) : 1) : 0;
        off[k] = in ? total : 0;
        total += 3ull * (unsigned long long)h[k] * (unsigned long long)w[k];
    }
    return true;
}

// The host's truncating float -> int32 conversion (cvttss2si): INT_MIN for a NaN and out of range.
// (Restated from model_ops.hip, whose text is fingerprinted, as texture.hip restates it.)
CR_DEV int host_f32_to_i32(float f)
{
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000;
}

CR_DEV const unsigned char *texel(const unsigned char *__restrict__ tex, int row, int colm, int tw)
{
    return tex + ((size_t)row * (size_t)tw + (size_t)colm) * 3;
}

// The Bilinear statement of crender_tex.h on one level (texture.hip's operation order).
CR_DEV void bilinear(const unsigned char *__restrict__ tex, int th, int tw, float tu, float tv, float c[3])
{
    const float fx = tu * (float)tw - 0.5f, fy = (1.0f - tv) * (float)th - 0.5f;
    const float x0 = floorf(fx), yf0 = floorf(fy);
    const float ax = fx - x0, ay = fy - yf0;
    const int cl = clipi(host_f32_to_i32(x0), 0, tw - 1), cr = clipi(host_f32_to_i32(x0 + 1.0f), 0, tw - 1);
    const int rt = clipi(host_f32_to_i32(yf0), 0, th - 1), rbm = clipi(host_f32_to_i32(yf0 + 1.0f), 0, th - 1);
    const unsigned char *t00 = texel(tex, rt, cl, tw), *t01 = texel(tex, rt, cr, tw);
    const unsigned char *t10 = texel(tex, rbm, cl, tw), *t11 = texel(tex, rbm, cr, tw);
    const float wx = 1.0f - ax, wy = 1.0f - ay;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        c[j] = ((float)t00[j] * wx + (float)t01[j] * ax) * wy + ((float)t10[j] * wx + (float)t11[j] * ax) * ay;
}

struct CornerUV {
    float u0, v0, u1, v1, u2, v2;
    float za, zb, zc;                // the corners' unprojected z (perspective mode)
    float ra, rb, rc;                // their refined reciprocals, valid if z_fast
    bool z_fast;                     // all three inside the division window of raster_math.h
};

// (u, v) of the integer pixel (X, Y) in projected triangle S: barycentrics, then the Affine or the
// Perspective statement.  The three points of a pixel divide by the same per-triangle numbers, so the
// quotients go through raster_math.h's shortcut (2): the refined reciprocal of a divisor is formed once
// and each quotient is the five-operation tail of the compiler's own expansion of `/`, which rounds
// identically inside the window; anything outside it (a zero barycentric on an edge, a NaN) takes `/`.
template <bool PERSPECTIVE>
CR_DEV void uv_at(const TriSetup &S, const CornerUV &k, int X, int Y, float &tu, float &tv)
{
    float n1, n2, n3, b1, b2, b3;
    numerators(S, X, Y, n1, n2, n3);
    quotients(S, n1, n2, n3, b1, b2, b3);
    if (PERSPECTIVE) {
        float q1, q2, q3;
        if (k.z_fast && in_div_window(b1) && in_div_window(b2) && in_div_window(b3)) {
            q1 = div_tail(b1, k.za, k.ra); q2 = div_tail(b2, k.zb, k.rb); q3 = div_tail(b3, k.zc, k.rc);
        } else {
            q1 = b1 / k.za; q2 = b2 / k.zb; q3 = b3 / k.zc;
        }
        const float s = (q1 + q2) + q3;
        const float nu = (k.u0 * q1 + k.u1 * q2) + k.u2 * q3, nv = (k.v0 * q1 + k.v1 * q2) + k.v2 * q3;
        if (in_div_window(s) && in_div_window(nu) && in_div_window(nv)) {
            const float r = refined_rcp(s);
            tu = div_tail(nu, s, r);
            tv = div_tail(nv, s, r);
        } else {
            tu = nu / s;
            tv = nv / s;
        }
    } else {
        tu = interp(k.u0, k.u1, k.u2, b1, b2, b3);
        tv = interp(k.v0, k.v1, k.v2, b1, b2, b3);
    }
}

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
