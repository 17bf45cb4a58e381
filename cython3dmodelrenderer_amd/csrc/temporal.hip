// temporal.hip — temporal anti-aliasing: a jittered frame resolved against its reprojected history
// (include/crender_taa.h states the arithmetic; this file keeps its operation order).
#include <math.h>

#include "common.h"
#include "../../include/crender_taa.h"

using namespace crender_detail;

#include "winner_pass.h"     // the tile frame, tile_grid; arg_error, rows_check

// The shape of k_dof_blur (dof.hip): a workgroup of 256 per tile of kTile x kTile pixels, looping over tiles, stages the
// tile plus a halo of one pixel into LDS once, a wavefront per staged row.  A row of a plane is contiguous in memory, so
// the wavefront's lanes walk its WORDS (102 of colour, 68 of velocity, 34 of z: unit-stride loads) and scatter them to
// planes of 34 x 34 words, one per component: three of colour, two of velocity and one of z where they are given.  A
// staged pixel off the frame or outside the strip holds NaNs: `v < lo`, `v > hi` and `z < best` all fail for a NaN, so it
// changes neither the box nor the dilation, as the contract's N(p) leaves it out.  The 27 box reads and the 9 depth reads
// of a pixel are ds_read_b32 at a 32-lane half's consecutive words: no bank conflicts.
//
// The history is gathered from global memory at the pixel's previous position: four texels, or one where no lane of the
// wavefront has a fraction (all velocities zero or whole pixels: a scalar branch).  Without a velocity plane the one texel
// is the pixel's own and the loads are unit-stride.

namespace {

constexpr int kTaaMaxGrid = 2048;            // workgroups of a launch: 8 per CU; the kernel loops over the other tiles
constexpr int kTaaPitch = kTile + 2;         // the tile and a halo of one pixel
constexpr int kTaaPlane = kTaaPitch * kTaaPitch;

// `n` words of row `gy` of a plane of C words a pixel, from pixel x0 - 1 on, scattered into C planes of LDS at `row`.
template <int C>
CR_DEV void stage_row(const float *__restrict__ g, float *__restrict__ s, int lane, bool row_in, int gy, int x0, int W, int row)
{
    for (int i = lane; i < kTaaPitch * C; i += 64) {
        const int sx = i / C, c = i - sx * C;
        const int gx = x0 - 1 + sx;
        float v = __builtin_nanf("");
        if (row_in && gx >= 0 && gx < W) v = g[((size_t)gy * (size_t)W + (size_t)gx) * C + c];
        s[c * kTaaPlane + row * kTaaPitch + sx] = v;
    }
}

CR_DEV float lerp_tap(float a, float b, float f) { return f == 0.0f ? a : a + (b - a) * f; }

template <bool VEL, bool DIL, bool CLAMP>
__global__ __launch_bounds__(kThreads) void k_taa_resolve(const float *__restrict__ cb, const float *__restrict__ hb,
                                                           const float *__restrict__ vb, const float *__restrict__ zb,
                                                           float keep, float *__restrict__ ob, int W, int y0, int y1,
                                                           int tiles_x, int ntiles)
{
    extern __shared__ float s_taa[];            // r, g, b; then vx, vy (VEL); then z (DIL): [34][34] each
    float *const s_c = s_taa, *const s_v = s_taa + 3 * kTaaPlane, *const s_z = s_taa + 5 * kTaaPlane;
    const auto [lane, wave, lx, ly] = tile_lane();
    const float xmax = (float)(W - 1), ymin = (float)y0, ymax = (float)(y1 - 1);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [x0, ty0] = tile_origin(tile, tiles_x, y0);
        // ---- stage the tile and its halo: a wavefront per row
        for (int sy = wave; sy < kTaaPitch; sy += kThreads / 64) {
            const int gy = ty0 - 1 + sy;
            const bool row_in = gy >= y0 && gy < y1;
            stage_row<3>(cb, s_c, lane, row_in, gy, x0, W, sy);
            if (VEL) stage_row<2>(vb, s_v, lane, row_in, gy, x0, W, sy);
            if (DIL) stage_row<1>(zb, s_z, lane, row_in, gy, x0, W, sy);
        }
        __syncthreads();
        // ---- the tile's pixels, 32 x 8 at a time
#pragma unroll 1
        for (int k = 0; k < kTile / kTileRows; ++k) {
            const int row = ly + k * kTileRows;
            const int x = x0 + lx, y = ty0 + row;
            const bool inside = x < W && y < y1;
            const size_t pix = (size_t)y * (size_t)W + (size_t)x;
            const int base = (row + 1) * kTaaPitch + lx + 1;
            const float c0 = s_c[base], c1 = s_c[kTaaPlane + base], c2 = s_c[2 * kTaaPlane + base];
            // 1. the velocity: the pixel's own, or that of the nearest pixel of the 3 x 3
            float vx = 0.0f, vy = 0.0f;
            if (VEL) {
                int at = base;
                if (DIL) {
                    float best = s_z[base];
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int n = base + dy * kTaaPitch + dx;
                            const float zn = s_z[n];
                            if (zn < best) { best = zn; at = n; }       // (p itself and every NaN fail)
                        }
                }
                vx = s_v[at];
                vy = s_v[kTaaPlane + at];
                if (!(__builtin_isfinite(vx) && __builtin_isfinite(vy))) { vx = 0.0f; vy = 0.0f; }
            }
            // 2. where it was
            const float px = (float)x - vx, py = (float)y - vy;
            const bool counts = inside && px >= 0.0f && px <= xmax && py >= ymin && py <= ymax;
            // 3. the history sample
            float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
            if (!VEL) {
                if (counts) {
                    const float *hp = hb + pix * 3;
                    h0 = hp[0]; h1 = hp[1]; h2 = hp[2];
                }
            } else {
                const float xf = floorf(px), yf = floorf(py);
                const float fx = px - xf, fy = py - yf;
                if (wave_any(counts && (fx != 0.0f || fy != 0.0f))) {       // a scalar branch: somebody needs four texels
                    if (counts) {
                        const int ix0 = (int)xf, iy0 = (int)yf;
                        const int ix1 = ix0 + 1 < W - 1 ? ix0 + 1 : W - 1, iy1 = iy0 + 1 < y1 - 1 ? iy0 + 1 : y1 - 1;
                        const float *r0 = hb + (size_t)iy0 * (size_t)W * 3, *r1 = hb + (size_t)iy1 * (size_t)W * 3;
                        const float *p00 = r0 + (size_t)ix0 * 3, *p01 = r0 + (size_t)ix1 * 3;
                        const float *p10 = r1 + (size_t)ix0 * 3, *p11 = r1 + (size_t)ix1 * 3;
                        const float a0 = p00[0], a1 = p00[1], a2 = p00[2], b0 = p01[0], b1 = p01[1], b2 = p01[2];
                        const float d0 = p10[0], d1 = p10[1], d2 = p10[2], e0 = p11[0], e1 = p11[1], e2 = p11[2];
                        const float t0 = lerp_tap(a0, b0, fx), t1 = lerp_tap(a1, b1, fx), t2 = lerp_tap(a2, b2, fx);
                        const float u0 = lerp_tap(d0, e0, fx), u1 = lerp_tap(d1, e1, fx), u2 = lerp_tap(d2, e2, fx);
                        h0 = lerp_tap(t0, u0, fy); h1 = lerp_tap(t1, u1, fy); h2 = lerp_tap(t2, u2, fy);
                    }
                } else if (counts) {                    // fx == 0 and fy == 0 in every lane: h = h00
                    const float *hp = hb + ((size_t)(int)yf * (size_t)W + (size_t)(int)xf) * 3;
                    h0 = hp[0]; h1 = hp[1]; h2 = hp[2];
                }
            }
            // 4. the box of the 3 x 3
            if (CLAMP) {
                float lo0 = c0, hi0 = c0, lo1 = c1, hi1 = c1, lo2 = c2, hi2 = c2;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int n = base + dy * kTaaPitch + dx;
                        const float v0 = s_c[n], v1 = s_c[kTaaPlane + n], v2 = s_c[2 * kTaaPlane + n];
                        if (v0 < lo0) lo0 = v0;
                        if (v0 > hi0) hi0 = v0;
                        if (v1 < lo1) lo1 = v1;
                        if (v1 > hi1) hi1 = v1;
                        if (v2 < lo2) lo2 = v2;
                        if (v2 > hi2) hi2 = v2;
                    }
                h0 = h0 < lo0 ? lo0 : (h0 > hi0 ? hi0 : h0);
                h1 = h1 < lo1 ? lo1 : (h1 > hi1 ? hi1 : h1);
                h2 = h2 < lo2 ? lo2 : (h2 > hi2 ? hi2 : h2);
            }
            // 5. the blend
            if (!inside) continue;
            float *op = ob + pix * 3;
            if (!counts) {
                op[0] = c0; op[1] = c1; op[2] = c2;         // the bits, copied
            } else {
                op[0] = c0 + (h0 - c0) * keep;
                op[1] = c1 + (h1 - c1) * keep;
                op[2] = c2 + (h2 - c2) * keep;
            }
        }
        __syncthreads();                                // the next tile's staging overwrites what the box read
    }
}

template <bool VEL, bool DIL, bool CLAMP>
void launch_taa(dim3 grid, size_t lds, hipStream_t stream, const float *cb, const float *hb, const float *vb, const float *zb,
                float keep, float *ob, int W, int y0, int y1, int tiles_x, int tiles)
{
    hipLaunchKernelGGL((k_taa_resolve<VEL, DIL, CLAMP>), grid, dim3(kThreads), lds, stream, cb, hb, vb, zb, keep, ob, W, y0, y1,
                       tiles_x, tiles);
}

}  // namespace

extern "C" {

int crender_taa_resolve(const float *d_color, const float *d_history, const float *d_velocity, const float *d_z, float blend,
                        float *d_out, int H, int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_taa_resolve";
    if (!d_color || !d_history || !d_out) return arg_error(E, "d_color, d_history or d_out is NULL");
    if (d_z && !d_velocity) return arg_error(E, "d_z without d_velocity");
    if (H < 1 || W < 1) return arg_error(E, "H or W is below 1");
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags & ~CRENDER_TAA_NO_CLAMP) return arg_error(E, "unknown flag bits");
    if (d_out == d_color || d_out == d_history) return arg_error(E, "d_out is d_color or d_history (the pass cannot run in place)");
    if (!isfinite(blend) || !(blend > 0.0f) || blend > 1.0f) return arg_error(E, "blend is not finite and in (0, 1]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (blend == 1.0f) {                                // the frame's rows, copied: they are contiguous
        const size_t first = (size_t)y0 * (size_t)W * 3, words = (size_t)(y1 - y0) * (size_t)W * 3;
        CR_HIP(hipMemcpyAsync(d_out + first, d_color + first, words * sizeof(float), hipMemcpyDeviceToDevice, s));
        return CRENDER_OK;
    }
    int tiles_x, tiles;
    if (W > (1 << 24) || H > (1 << 24)) return arg_error(E, "H or W is too large");      // (float)x and (float)y are exact
    if (int rc = tile_grid(E, W, y0, y1, tiles_x, tiles)) return rc;
    const bool vel = d_velocity != nullptr, dil = d_z != nullptr, clamp = !(flags & CRENDER_TAA_NO_CLAMP);
    const size_t lds = (size_t)(3 + (vel ? 2 : 0) + (dil ? 1 : 0)) * kTaaPlane * sizeof(float);
    const dim3 grid((unsigned)(tiles < kTaaMaxGrid ? tiles : kTaaMaxGrid));
    const float keep = 1.0f - blend;
    auto *const launch = !vel ? (clamp ? launch_taa<false, false, true> : launch_taa<false, false, false>)
                         : !dil ? (clamp ? launch_taa<true, false, true> : launch_taa<true, false, false>)
                                : (clamp ? launch_taa<true, true, true> : launch_taa<true, true, false>);
    launch(grid, lds, s, d_color, d_history, d_velocity, d_z, keep, d_out, W, y0, y1, tiles_x, tiles);
    CR_LAUNCH_CHECK("k_taa_resolve");
    return CRENDER_OK;
}

}  // extern "C"
