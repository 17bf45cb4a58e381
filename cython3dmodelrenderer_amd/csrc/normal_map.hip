// normal_map.hip — normal mapping: a tangent-space map from a height map, and the deferred pass that perturbs the
// normal plane (include/crender_nmap.h states the arithmetic; this file keeps its operation order).
#include <math.h>

#include "common.h"
#include "../../include/crender_nmap.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, winner_triangle, the texel fetches, pass_grid, frame_checks

// ---- normal mapping (crender_nmap_from_height, crender_nmap_shade) ------------------------------------------------
// A deferred pass that rewrites the NORMAL plane for the covered pixels, once and right after the draw: every pass that
// lights a pixel reads that plane (the illumination pass, the fused light of the texture passes and of the resolve,
// k_phong_shade, k_ao_shade), so all of them get the bumps without a change.  The shape of k_tex_shade (texture.hip): a
// pixel per work item, an 8 x 8 block of pixels per wavefront, a grid-stride loop over row blocks; a wavefront whose 64
// winners are all background leaves after its one load.  A covered pixel projects its winner, takes (u, v) from the
// rasterizer's barycentrics (for the trilinear filter also at its right and lower neighbour: two more barycentric
// triples of the same triangle, whose nine edge constants the compiler keeps), samples the map, builds the tangent frame
// of the triangle from its unprojected corners and its uv, turns it around the stored normal and stores the sum.  What
// the pass needs of the mip unit — the chain's layout and the level of a footprint, crender_mip.h's statements — is
// restated here: that unit's headers are its own.  The level offsets travel by value in the kernel's arguments.

namespace {

constexpr int kNmapMaxLevels = 16;           // a side is at most 65 535
enum { kNmapNearest = 0, kNmapBilinear = 1, kNmapTrilinear = 2 };

// The map of a call: its size and, for a chain, where each level starts (crender_mip_build's layout).
struct NmapChain {
    unsigned long long off[kNmapMaxLevels];
    int mh, mw, L;
};

NmapChain nmap_chain(int mh, int mw, bool chain)
{
    NmapChain M{};
    M.mh = mh;
    M.mw = mw;
    M.L = 1;
    if (chain) {
        const int side = mh > mw ? mh : mw;
        M.L = 0;
        while ((side >> M.L) > 0) ++M.L;     // 1 + floor(log2(side))
        unsigned long long total = 0;
        for (int k = 0; k < M.L; ++k) {
            const int h = (mh >> k) > 1 ? (mh >> k) : 1, w = (mw >> k) > 1 ? (mw >> k) : 1;
            M.off[k] = total;
            total += 3ull * (unsigned long long)h * (unsigned long long)w;
        }
    }
    return M;
}

// The Level statement of crender_mip.h: the lower level l0 and the weight f of the one above it.
CR_DEV void nmap_level(float rho, int L, int &l0, float &f)
{
    l0 = 0;
    f = 0.0f;
    if (rho > 1.0f) {
        if (!(rho < (float)(1u << (L - 1)))) {
            l0 = L - 1;
        } else {
            // 1 < rho < 2^15: the exponent field is the level, the significand scaled back by the exact power is 1 + f
            l0 = (int)(__float_as_uint(rho) >> 23) - 127;
            f = rho * __uint_as_float((uint32_t)(127 - l0) << 23) - 1.0f;
        }
    }
}

// (u, v) of the integer pixel (x, y) in projected triangle X: the Affine or the Perspective statement of crender_tex.h.
template <bool PERSPECTIVE>
CR_DEV void nmap_uv(const TriXYZ &X, float za, float zb, float zc, const float w[6], int x, int y, float &tu, float &tv)
{
    float b1, b2, b3;
    barycentric(X, x, y, b1, b2, b3);
    if (PERSPECTIVE) {
        const float q1 = b1 / za, q2 = b2 / zb, q3 = b3 / zc;
        const float s = (q1 + q2) + q3;
        tu = ((w[0] * q1 + w[2] * q2) + w[4] * q3) / s;
        tv = ((w[1] * q1 + w[3] * q2) + w[5] * q3) / s;
    } else {
        tu = interp(w[0], w[2], w[4], b1, b2, b3);
        tv = interp(w[1], w[3], w[5], b1, b2, b3);
    }
}

CR_DEV float nmap_dot(const float a[3], const float b[3])
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

template <bool PERSPECTIVE, int FILTER>
__global__ __launch_bounds__(kThreads) void k_nmap_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                          int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                          const float *__restrict__ uv,
                                                          const unsigned char *__restrict__ map, NmapChain M,
                                                          float strength, float *__restrict__ nb, int W, int y0, int y1,
                                                          int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!wave_any(px.covered)) continue;        // a scalar branch: the whole wavefront leaves
        if (!px.covered) continue;
        float raw[3][3];
        const TriXYZ X = winner_triangle(tri, px.t, P, raw);
        const float *wp = uv + px.orig * 6;
        const float w[6] = {wp[0], wp[1], wp[2], wp[3], wp[4], wp[5]};
        // ---- 1, 2: the sample
        float tu, tv, s[3];
        nmap_uv<PERSPECTIVE>(X, raw[0][2], raw[1][2], raw[2][2], w, px.x, px.y, tu, tv);
        if (FILTER == kNmapTrilinear) {
            float ux, vx, uy, vy;
            nmap_uv<PERSPECTIVE>(X, raw[0][2], raw[1][2], raw[2][2], w, px.x + 1, px.y, ux, vx);
            nmap_uv<PERSPECTIVE>(X, raw[0][2], raw[1][2], raw[2][2], w, px.x, px.y + 1, uy, vy);
            const float fmw = (float)M.mw, fmh = (float)M.mh;
            const float dudx = (ux - tu) * fmw, dvdx = (vx - tv) * fmh;
            const float dudy = (uy - tu) * fmw, dvdy = (vy - tv) * fmh;
            const float rx = dudx * dudx + dvdx * dvdx;
            const float ry = dudy * dudy + dvdy * dvdy;
            const float r2 = (rx >= ry) ? rx : ry;
            const float rho = sqrtf(r2);
            int l0;
            float f;
            nmap_level(rho, M.L, l0, f);
            const int hl = max(1, M.mh >> l0), wl = max(1, M.mw >> l0);
            bilinear(map + (l0 ? M.off[l0] : 0ull), hl, wl, tu, tv, s);
            if (f != 0.0f) {         // (only between two levels: l0 + 1 <= L - 1)
                float up[3];
                bilinear(map + M.off[l0 + 1], max(1, hl >> 1), max(1, wl >> 1), tu, tv, up);
                const float g = 1.0f - f;
#pragma unroll
                for (int j = 0; j < 3; ++j) s[j] = s[j] * g + up[j] * f;
            }
        } else if (FILTER == kNmapBilinear) {
            bilinear(map, M.mh, M.mw, tu, tv, s);
        } else {
            const int row = clipi(host_f32_to_i32((1.0f - tv) * (float)M.mh), 0, M.mh - 1);
            const int colm = clipi(host_f32_to_i32(tu * (float)M.mw), 0, M.mw - 1);
            const unsigned char *p = texel(map, row, colm, M.mw);
            s[0] = (float)p[0]; s[1] = (float)p[1]; s[2] = (float)p[2];
        }
        float m[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            m[j] = (s[j] - 128.0f) / 127.0f;
            m[j] = m[j] < -1.0f ? -1.0f : m[j];
        }
        const float mx = m[0] * strength, my = m[1] * strength, mz = m[2];
        // ---- 3: the tangent frame of the triangle
        const float du1 = w[2] - w[0], dv1 = w[3] - w[1], du2 = w[4] - w[0], dv2 = w[5] - w[1];
        const float det = du1 * dv2 - du2 * dv1;
        const float sg = det < 0.0f ? -1.0f : 1.0f;
        float Tt[3], Bt[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float e1 = raw[1][j] - raw[0][j], e2 = raw[2][j] - raw[0][j];
            Tt[j] = (e1 * dv2 - e2 * dv1) * sg;
            Bt[j] = (e2 * du1 - e1 * du2) * sg;
        }
        // ---- 4: the frame around the stored normal
        float *np_ = nb + px.pix * 3;
        const float n[3] = {np_[0], np_[1], np_[2]};
        const float nl = sqrtf(nmap_dot(n, n));
        const float Nu[3] = {n[0] / nl, n[1] / nl, n[2] / nl};
        const float d = nmap_dot(Nu, Tt);
        const float Tp[3] = {Tt[0] - Nu[0] * d, Tt[1] - Nu[1] * d, Tt[2] - Nu[2] * d};
        const float tl = sqrtf(nmap_dot(Tp, Tp));
        const float Tu[3] = {Tp[0] / tl, Tp[1] / tl, Tp[2] / tl};
        float Bp[3] = {Nu[1] * Tu[2] - Nu[2] * Tu[1], Nu[2] * Tu[0] - Nu[0] * Tu[2], Nu[0] * Tu[1] - Nu[1] * Tu[0]};
        if (nmap_dot(Bp, Bt) < 0.0f) {
            Bp[0] = -Bp[0]; Bp[1] = -Bp[1]; Bp[2] = -Bp[2];
        }
        // ---- 5, 6: the result, where there is a frame and something to tilt by (false for every NaN)
        const bool tilt = mx < 0.0f || mx > 0.0f || my < 0.0f || my > 0.0f;
        if ((det > 0.0f || det < 0.0f) && nl > 0.0f && tl > 0.0f && tilt) {
#pragma unroll
            for (int j = 0; j < 3; ++j) np_[j] = (Tu[j] * mx + Bp[j] * my) + Nu[j] * mz;
        }
    }
}

// A texel per work item in a grid-stride loop: the statements of crender_nmap_from_height.
__global__ __launch_bounds__(kThreads) void k_nmap_from_height(const uint8_t *__restrict__ hm, int mh, int mw, float k,
                                                                int wrap, uint8_t *__restrict__ out)
{
    const size_t n = (size_t)mh * (size_t)mw;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const int r = (int)(i / (size_t)mw), c = (int)(i - (size_t)r * (size_t)mw);
        int cl = c - 1, cr = c + 1, ru = r - 1, rd = r + 1;
        if (wrap) {
            cl = cl < 0 ? mw - 1 : cl;
            cr = cr >= mw ? 0 : cr;
            ru = ru < 0 ? mh - 1 : ru;
            rd = rd >= mh ? 0 : rd;
        } else {
            cl = cl < 0 ? 0 : cl;
            cr = cr >= mw ? mw - 1 : cr;
            ru = ru < 0 ? 0 : ru;
            rd = rd >= mh ? mh - 1 : rd;
        }
        const uint8_t *row = hm + (size_t)r * (size_t)mw;
        const float gx = (float)((int)row[cr] - (int)row[cl]) * k;
        const float gy = (float)((int)hm[(size_t)ru * (size_t)mw + (size_t)c] - (int)hm[(size_t)rd * (size_t)mw + (size_t)c]) * k;
        const float ln = sqrtf((gx * gx + gy * gy) + 1.0f);
        const float v[3] = {-gx / ln, -gy / ln, 1.0f / ln};
        uint8_t *o = out + i * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float b = rintf(v[j] * 127.0f + 128.0f);
            o[j] = (uint8_t)(int)(!(b > 0.0f) ? 0.0f : (b > 255.0f ? 255.0f : b));      // (a NaN gives 0)
        }
    }
}

}  // namespace

extern "C" {

int crender_nmap_from_height(const uint8_t *d_height, int mh, int mw, float scale, unsigned flags, uint8_t *d_map,
                             void *stream)
{
    const char *const E = "crender_nmap_from_height";
    if (!d_height || !d_map) return arg_error(E, "d_height or d_map is NULL");
    if (mh < 1 || mw < 1 || mh > 65535 || mw > 65535) return arg_error(E, "mh or mw is not 1 .. 65535");
    if (!isfinite(scale)) return arg_error(E, "scale is not finite");
    if (flags & ~(unsigned)CRENDER_NMAP_WRAP) return arg_error(E, "unknown flag bits");
    const float k = scale / 255.0f;
    hipLaunchKernelGGL(k_nmap_from_height, dim3(grid_for((size_t)mh * (size_t)mw, 16384)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_height, mh, mw, k, (flags & CRENDER_NMAP_WRAP) ? 1 : 0, d_map);
    CR_LAUNCH_CHECK("k_nmap_from_height");
    return CRENDER_OK;
}

int crender_nmap_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of, const float *P16,
                       const float *d_uv, const uint8_t *d_map, int mh, int mw, float strength, float *d_normal, int H,
                       int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_nmap_shade";
    if (!d_winner || !P16 || !d_map || !d_normal) return arg_error(E, "d_winner, P16, d_map or d_normal is NULL");
    if (int rc = frame_checks(E, T, d_tri && d_uv, H, W, "d_tri or d_uv is NULL with T > 0")) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (mh < 1 || mw < 1 || mh > 65535 || mw > 65535) return arg_error(E, "mh or mw is not 1 .. 65535");
    if (!isfinite(strength)) return arg_error(E, "strength is not finite");
    const bool persp = flags & CRENDER_NMAP_PERSPECTIVE, bilin = flags & CRENDER_NMAP_BILINEAR, chain = flags & CRENDER_NMAP_CHAIN;
    if (flags & ~(unsigned)(CRENDER_NMAP_PERSPECTIVE | CRENDER_NMAP_BILINEAR | CRENDER_NMAP_CHAIN))
        return arg_error(E, "unknown flag bits");
    if (chain && bilin) return arg_error(E, "CRENDER_NMAP_CHAIN with CRENDER_NMAP_BILINEAR");
    if (T == 0) return CRENDER_OK;
    // [perspective][filter]
    static constexpr decltype(&k_nmap_shade<false, kNmapNearest>) kernels[2][3] = {
        {k_nmap_shade<false, kNmapNearest>, k_nmap_shade<false, kNmapBilinear>, k_nmap_shade<false, kNmapTrilinear>},
        {k_nmap_shade<true, kNmapNearest>, k_nmap_shade<true, kNmapBilinear>, k_nmap_shade<true, kNmapTrilinear>}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[persp][chain ? kNmapTrilinear : (bilin ? kNmapBilinear : kNmapNearest)], G.grid,
                       dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner, d_tri, T, d_pos_of,
                       make_proj(P16, W, H), d_uv, d_map, nmap_chain(mh, mw, chain), strength, d_normal, W, y0, y1,
                       G.row_blocks);
    CR_LAUNCH_CHECK("k_nmap_shade");
    return CRENDER_OK;
}

}  // extern "C"
