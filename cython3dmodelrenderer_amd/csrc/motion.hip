// motion.hip — per-pixel motion vectors against an earlier pose, and a motion blur that gathers along them
// (include/crender_motion.h states the arithmetic; this file keeps its operation order).
#include <math.h>

#include "common.h"
#include "../../include/crender_motion.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, winner_triangle, pass_grid; the tile frame, tile_grid; frame_checks, rows_check

// ---- motion vectors (crender_motion_vectors) ----
// The shape of k_shadow_shade (shadow.hip): a pixel per work item, an 8 x 8 block of pixels per wavefront, a grid-stride
// loop over row blocks.  What is blended across the winner's triangle is the PREVIOUS pose's three corners (36 B per
// winner, gathered beside the 36 B of its own: 72 B per distinct winner), and the blend goes through the frame's own
// projection: where the surface point was on the screen.  Every pixel of the rows stores its 8 B, the background zeros.
//
// ---- motion blur (crender_motion_blur) ----
// The shape of k_dof_blur (dof.hip): a workgroup of 256 per tile of kTile x kTile pixels, looping over tiles, stages the
// tile plus a halo of max_radius into LDS once, a wavefront per staged row with unit-stride loads, FIVE words a pixel:
// il (the reciprocal of the half velocity's length: the one division, per STAGED pixel), the view depth zv and the three
// colours, in five planes of (32 + 2 R)^2 words (62.7 KB at R = 12).  A staged pixel off the frame or outside the strip
// gets zv = NaN: every alpha with it is a NaN, `alpha > 0` fails, and it contributes nowhere.
//
// The dominant pixel (largest l, the first in frame order among equals) is reduced while staging: a non-negative l's bits
// order as ints and the staged index orders as the frame does, so a wavefront's own (max bits, then min index) by DPP and
// two LDS words per wavefront.  A tile whose dominant l is not above 1/2 copies its pixels.  Otherwise the first 32 work
// items make the table of N (LDS offset, dist) entries from the dominant pixel's velocity, read again from the plane (a
// uniform address), and every pixel walks the SAME taps: a tap is two ds_read_b32 (il and zv of q) at the lane's base
// plus an offset uniform for the workgroup, so a lane group reads 32 consecutive words: no bank conflicts under any
// pitch.  The taps go four at a time, eight reads in flight, and only if a lane of the wavefront takes one of the four (a
// scalar branch) their colours are read.  The sums are made in the taps' own order.  No tap divides or takes a root.

namespace {

// (hx, hy), the half velocity of a pixel clamped to Rf, and l, its length: the contract's statement, for the staged
// pixels and again for the dominant one.
CR_DEV void half_velocity(float vx, float vy, float Rf, float &hx, float &hy, float &l)
{
    if (!(__builtin_isfinite(vx) && __builtin_isfinite(vy))) { vx = 0.0f; vy = 0.0f; }
    hx = vx * 0.5f;
    hy = vy * 0.5f;
    l = sqrtf(hx * hx + hy * hy);
    if (l > Rf) {
        const float k = Rf / l;
        hx = hx * k;
        hy = hy * k;
        l = Rf;
    }
}

__global__ __launch_bounds__(kThreads) void k_motion_vectors(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                              int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                              const float *__restrict__ ptri, float exposure,
                                                              float *__restrict__ vb, int W, int y0, int y1, int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!px.inside) continue;
        float vx = 0.0f, vy = 0.0f;
        if (px.covered) {
            float raw[3][3];
            const TriXYZ X = winner_triangle(tri, px.t, P, raw);
            float b1, b2, b3;
            barycentric(X, px.x, px.y, b1, b2, b3);
            const float q1 = b1 / raw[0][2], q2 = b2 / raw[1][2], q3 = b3 / raw[2][2];
            const float s = (q1 + q2) + q3;
            const float *c = ptri + px.orig * 9;        // the previous pose, in the caller's order
            float p[3];
            p[0] = ((c[0] * q1 + c[3] * q2) + c[6] * q3) / s;
            p[1] = ((c[1] * q1 + c[4] * q2) + c[7] * q3) / s;
            p[2] = ((c[2] * q1 + c[5] * q2) + c[8] * q3) / s;
            if (p[2] > 0.0f) {                          // (behind the camera, or NaN: no velocity)
                project_vertex(P, p);
                const float ux = ((float)px.x - p[0]) * exposure, uy = ((float)px.y - p[1]) * exposure;
                if (__builtin_isfinite(ux) && __builtin_isfinite(uy)) { vx = ux; vy = uy; }
            }
        }
        float *vp = vb + px.pix * 2;
        vp[0] = vx;
        vp[1] = vy;
    }
}

constexpr int kBlurMaxGrid = 2048;           // workgroups of a launch: 8 per CU; the kernel loops over the other tiles
constexpr int kBlurTaps = CRENDER_MOTION_MAX_TAPS;
constexpr int kBlurMore = 2 * (kThreads / 64) + 2 * kBlurTaps;     // the words of LDS after the five planes

// The constants of a call.
struct BlurParams {
    float p10, p14, Rf, isoft;
    int R, N;
};

CR_DEV float clamp01(float a) { return a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a); }      // (a NaN stays a NaN)

CR_DEV float cone(float m)
{
    const float t = 1.0f - m;
    return t > 0.0f ? t : 0.0f;
}

CR_DEV float cylinder(float m)
{
    const float u = clamp01((m - 0.95f) * 10.0f);
    return 1.0f - (u * u) * (3.0f - 2.0f * u);
}

__global__ __launch_bounds__(kThreads) void k_motion_blur(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                           int64_t T, const float *__restrict__ cb,
                                                           const float *__restrict__ vb, BlurParams A,
                                                           float *__restrict__ ob, int W, int y0, int y1, int tiles_x,
                                                           int ntiles)
{
    extern __shared__ float s_mb[];             // il, zv, r, g, b: [kTile + 2R][kTile + 2R] each; then s_top, s_off, s_dist
    const int R = A.R, pitch = kTile + 2 * R, plane = pitch * pitch;
    float *const s_il = s_mb, *const s_zv = s_mb + plane;
    float *const s_c0 = s_mb + 2 * plane, *const s_c1 = s_mb + 3 * plane, *const s_c2 = s_mb + 4 * plane;
    int *const s_top = reinterpret_cast<int *>(s_mb + 5 * plane);      // per wavefront: the bits of its largest l, and where
    int *const s_off = s_top + 2 * (kThreads / 64);                     // per tap: oy * pitch + ox; 0: skipped
    float *const s_dist = reinterpret_cast<float *>(s_off + kBlurTaps);
    const auto [lane, wave, lx, ly] = tile_lane();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [x0, ty0] = tile_origin(tile, tiles_x, y0);
        // ---- stage il, zv and the colours of the tile and its halo: a wavefront per row (pitch <= 56 columns)
        int top = -1, top_at = 0x7FFFFFFF;      // an l is >= +0: its bits order as ints; -1: no pixel of the frame yet
        for (int sy = wave; sy < pitch; sy += kThreads / 64) {
            const int gy = ty0 - R + sy;
            const bool row_in = gy >= y0 && gy < y1;
            for (int sx = lane; sx < pitch; sx += 64) {
                const int gx = x0 - R + sx;
                const int at = sy * pitch + sx;
                float il = 2.0f, zv = __builtin_nanf(""), c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
                if (row_in && gx >= 0 && gx < W) {
                    const size_t pix = (size_t)gy * (size_t)W + (size_t)gx;
                    const int32_t w = win[pix];
                    const float z = zb[pix];
                    const float *cp = cb + pix * 3;
                    const float *vp = vb + pix * 2;
                    c0 = cp[0]; c1 = cp[1]; c2 = cp[2];
                    float hx, hy, l;
                    half_velocity(vp[0], vp[1], A.Rf, hx, hy, l);
                    il = 1.0f / (l > 0.5f ? l : 0.5f);
                    zv = (w >= 0 && w < T) ? A.p14 / (z - A.p10) : CRENDER_MOTION_FAR;
                    const int bits = __float_as_int(l);
                    if (bits > top) { top = bits; top_at = at; }       // (a work item's `at` ascends: the first stays)
                }
                s_il[at] = il;
                s_zv[at] = zv;
                s_c0[at] = c0; s_c1[at] = c1; s_c2[at] = c2;
            }
        }
        {
            const int wave_top = wave_reduce<true>(top);
            const int wave_at = wave_reduce<false>(top == wave_top ? top_at : 0x7FFFFFFF);
            if (lane == 0) { s_top[2 * wave] = wave_top; s_top[2 * wave + 1] = wave_at; }
        }
        __syncthreads();
        int all = s_top[0], all_at = s_top[1];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) {
            const int b = s_top[2 * w], a = s_top[2 * w + 1];
            if (b > all || (b == all && a < all_at)) { all = b; all_at = a; }
        }
        all = __builtin_amdgcn_readfirstlane(all);
        all_at = __builtin_amdgcn_readfirstlane(all_at);
        // the tile's own first pixel is on the frame and in the strip, so a dominant pixel exists; guarded all the same
        const bool walk = all >= 0 && all_at < plane && __int_as_float(all) > 0.5f;
        if (walk) {
            // ---- the taps of this tile, from the dominant pixel's half velocity: uniform for the workgroup
            if ((int)threadIdx.x < kBlurTaps) {
                const int i = (int)threadIdx.x;
                int off = 0;
                float dist = 0.0f;
                if (i < A.N) {
                    const int sy = all_at / pitch, sx = all_at - sy * pitch;
                    const size_t pix = (size_t)(ty0 - R + sy) * (size_t)W + (size_t)(x0 - R + sx);
                    float Dx, Dy, l;
                    half_velocity(vb[pix * 2], vb[pix * 2 + 1], A.Rf, Dx, Dy, l);
                    const float tau = (float)(2 * i + 1 - A.N) / (float)A.N;
                    int ox = (int)rintf(Dx * tau), oy = (int)rintf(Dy * tau);
                    ox = ox < -R ? -R : (ox > R ? R : ox);      // (they are within: kept as a guard of the LDS offsets)
                    oy = oy < -R ? -R : (oy > R ? R : oy);
                    off = oy * pitch + ox;                      // 0 only for (0, 0): |ox| <= R < pitch / 2
                    dist = sqrtf((float)(ox * ox + oy * oy));
                }
                s_off[i] = off;
                s_dist[i] = dist;
            }
            __syncthreads();
        }
        // ---- the tile's pixels, 32 x 8 at a time
#pragma unroll 1
        for (int k = 0; k < kTile / kTileRows; ++k) {
            const int row = ly + k * kTileRows;
            const int x = x0 + lx, y = ty0 + row;
            const bool inside = x < W && y < y1;
            const size_t pix = (size_t)y * (size_t)W + (size_t)x;
            const int base = (row + R) * pitch + lx + R;
            const float own0 = s_c0[base], own1 = s_c1[base], own2 = s_c2[base];
            float *op = ob + pix * 3;
            if (!walk) {                                // a scalar branch: nothing around here moves
                if (inside) { op[0] = own0; op[1] = own1; op[2] = own2; }
                continue;
            }
            const float ilp = s_il[base], zvp = s_zv[base];
            float Sw = ilp, S0 = own0 * ilp, S1 = own1 * ilp, S2 = own2 * ilp;
            bool any = false;                           // a tap was taken
            // four taps at a time: their reads of il and zv are in flight together, then the colours of the four if a
            // lane takes any of them, then the sums in the taps' own order.  (The table holds 32 entries, those from N on
            // skipped.)
            for (int i0 = 0; i0 < A.N; i0 += 4) {
                float al[4];
                int offs[4];
                bool take[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int off = s_off[i0 + j];
                    const float d = s_dist[i0 + j];
                    const float ilq = s_il[base + off], zvq = s_zv[base + off];
                    const float mq = d * ilq, mp = d * ilp;
                    const float fg = clamp01(1.0f - (zvq - zvp) * A.isoft);
                    const float bg = clamp01(1.0f - (zvp - zvq) * A.isoft);
                    al[j] = (fg * cone(mq) + bg * cone(mp)) + 2.0f * (cylinder(mq) * cylinder(mp));
                    offs[j] = off;
                    take[j] = inside && off != 0 && al[j] > 0.0f;       // (every NaN fails)
                }
                if (!wave_any(take[0] || take[1] || take[2] || take[3])) continue;    // a scalar branch: nobody reads the colours
                float q0[4], q1[4], q2[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int at = base + offs[j];
                    q0[j] = s_c0[at]; q1[j] = s_c1[at]; q2[j] = s_c2[at];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (take[j]) {
                        Sw = Sw + al[j];
                        S0 = S0 + al[j] * q0[j];
                        S1 = S1 + al[j] * q1[j];
                        S2 = S2 + al[j] * q2[j];
                        any = true;
                    }
                }
            }
            if (!inside) continue;
            if (!any) {
                op[0] = own0; op[1] = own1; op[2] = own2;      // the bits, copied
            } else {
                op[0] = S0 / Sw; op[1] = S1 / Sw; op[2] = S2 / Sw;
            }
        }
        __syncthreads();                                // the next tile's staging overwrites what the taps read
    }
}

}  // namespace

extern "C" {

int crender_motion_vectors(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                           const float *P16, const float *d_prev_tri, float exposure, float *d_velocity, int H, int W,
                           int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_motion_vectors";
    if (!d_winner || !P16 || !d_velocity) return arg_error(E, "d_winner, P16 or d_velocity is NULL");
    if (int rc = frame_checks(E, T, d_tri && d_prev_tri, H, W, "d_tri or d_prev_tri is NULL with T > 0")) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags) return arg_error(E, "unknown flag bits");
    if (!isfinite(exposure) || exposure < 0.0f) return arg_error(E, "exposure is not finite and 0 or above");
    // (T == 0: no winner is valid and no triangle is read; the rows are written as zeros)
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(k_motion_vectors, G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner, d_tri, T,
                       d_pos_of, make_proj(P16, W, H), d_prev_tri, exposure, d_velocity, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_motion_vectors");
    return CRENDER_OK;
}

int crender_motion_blur(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                        const float *P16, const float *d_color, const float *d_velocity, int max_radius, int taps, float soft,
                        float *d_out, int H, int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_motion_blur";
    (void)d_tri;
    (void)d_pos_of;
    if (!d_winner || !d_z || !P16 || !d_color || !d_velocity || !d_out)
        return arg_error(E, "d_winner, d_z, P16, d_color, d_velocity or d_out is NULL");
    if (int rc = frame_checks(E, T, true, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags) return arg_error(E, "unknown flag bits");
    if (d_out == d_color) return arg_error(E, "d_out is d_color (the pass cannot run in place)");
    if (int rc = projection_shape_check(E, P16)) return rc;
    if (max_radius < 1 || max_radius > CRENDER_MOTION_MAX_RADIUS) return arg_error(E, "max_radius is not 1 .. 12");
    if (taps < 1 || taps > CRENDER_MOTION_MAX_TAPS) return arg_error(E, "taps is not 1 .. 32");
    if (!isfinite(soft) || !(soft > 0.0f)) return arg_error(E, "soft is not finite and positive");
    int tiles_x, tiles;
    if (int rc = tile_grid(E, W, y0, y1, tiles_x, tiles)) return rc;
    const size_t lds = tile_lds_bytes(max_radius) * 5 + kBlurMore * 4;
    if (lds > 65536) return arg_error(E, "max_radius needs more LDS than a workgroup has");      // (it does not: a guard)
    const BlurParams A = {P16[10], P16[14], (float)max_radius, 1.0f / soft, max_radius, taps};
    hipLaunchKernelGGL(k_motion_blur, dim3((unsigned)(tiles < kBlurMaxGrid ? tiles : kBlurMaxGrid)), dim3(kThreads), lds,
                       static_cast<hipStream_t>(stream), d_winner, d_z, T, d_color, d_velocity, A, d_out, W, y0, y1, tiles_x,
                       tiles);
    CR_LAUNCH_CHECK("k_motion_blur");
    return CRENDER_OK;
}

}  // extern "C"
