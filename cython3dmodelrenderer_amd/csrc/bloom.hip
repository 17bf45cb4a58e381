// bloom.hip — bloom and tone mapping as a separable post-process over any float32 image
// (include/crender_bloom.h states the arithmetic; this file keeps its operation order).
#include <math.h>

#include "common.h"
#include "../../include/crender_bloom.h"

using namespace crender_detail;

#include "winner_pass.h"     // the tile frame (kTile, TileLane, tile_origin), tile_grid, frame_checks, rows_check

// ---- bloom (crender_bloom) ----
// A glow around what is brighter than a threshold, and the curve that brings the range back into 0 .. 255: a post-process
// over ANY float32 image [H][W][3], not over the winner plane.  Separable: the bright values are blurred along the rows
// into a scratch plane hb (k_bloom_rows), hb is blurred along the columns, composited over the source, tone mapped,
// clamped and stored (k_bloom_finish): 2 (2 R + 1) taps a pixel where a gather walks (2 R + 1)^2.
//
// Geometry.  k_ao_shade's (ao.hip): a workgroup of 256 per tile of kTile x kTile pixels, looping over tiles; 256 work
// items are 32 x 8 pixels, a wavefront two rows of 32.  A kernel stages what its taps read once into THREE planes of
// LDS, one per channel, so that a tap is one ds_read_b32 per channel at the lane's base plus a wave-uniform offset and a
// lane group reads 32 consecutive words: free of bank conflicts.  k_bloom_rows stages 32 rows x (32 + 2 R) columns of
// bright values (the bright pass is made as they are staged: one division per staged bright pixel), k_bloom_finish
// (32 + 2 R) rows x 32 columns of hb: 3 * 32 * (32 + 2 R) words each, 13 056 B at R = 1, 18 432 B at 8, 36 864 B at 32.
// A staged value off the frame or outside the strip is +0.
//
// Work.  The taps are walked in the contract's order, -R .. R, four at a time so that twelve reads are in flight, each
// tap one multiply and one add per channel; the weights are read from the kernel arguments at a wave-uniform index.
// Dark work is skipped, which cannot change a bit (finite weights: a sum of products with +-0 from +0 is +0): in
// k_bloom_rows a wavefront stages the rows it walks, two at a time, and walks a pair only if one of its staged values
// is not +-0 (a scalar branch); in k_bloom_finish the workgroup ORs what its wavefronts staged through four words of
// LDS, and a dark tile goes straight to the copy of rule 4 and the tone stage.

namespace {

constexpr int kBloomMaxGrid = 2048;          // workgroups of a launch: 8 per CU; the kernels loop over the other tiles
constexpr int kBloomTaps = 4;                // taps whose reads are in flight together

// The constants of a call; w[k] is the weight of the taps at distance k.
struct BloomParams {
    float threshold, intensity, exposure, inv255, iw2, clamp;
    int R, H, tone, reinhard, gamma2, flip;
    float w[CRENDER_BLOOM_MAX_RADIUS + 1];
};

__device__ inline bool bloom_lit(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) != 0u; }      // not +-0

// The 2 R + 1 taps of one pixel along one direction: plane words base, base + step, ...; the sums start from +0.
__device__ inline void bloom_walk(const float *p0, const float *p1, const float *p2, int base, int step,
                                  const BloomParams &A, float &a0, float &a1, float &a2)
{
    const int R = A.R, n = 2 * R + 1;
    int t = 0;
    for (; t + kBloomTaps <= n; t += kBloomTaps) {
        float v0[kBloomTaps], v1[kBloomTaps], v2[kBloomTaps];
#pragma unroll
        for (int j = 0; j < kBloomTaps; ++j) {
            const int at = base + (t + j) * step;
            v0[j] = p0[at]; v1[j] = p1[at]; v2[j] = p2[at];
        }
#pragma unroll
        for (int j = 0; j < kBloomTaps; ++j) {
            const int d = t + j - R;
            const float w = A.w[d < 0 ? -d : d];
            a0 = a0 + w * v0[j];
            a1 = a1 + w * v1[j];
            a2 = a2 + w * v2[j];
        }
    }
    for (; t < n; ++t) {                        // the last one or three taps
        const int at = base + t * step, d = t - R;
        const float w = A.w[d < 0 ? -d : d];
        a0 = a0 + w * p0[at];
        a1 = a1 + w * p1[at];
        a2 = a2 + w * p2[at];
    }
}

__global__ __launch_bounds__(kThreads) void k_bloom_rows(const float *__restrict__ src, BloomParams A,
                                                          float *__restrict__ hb, int W, int y0, int y1, int tiles_x,
                                                          int ntiles)
{
    extern __shared__ float s_bloom[];          // the bright r, g, b: [kTile][kTile + 2R] each
    const int R = A.R, pitch = kTile + 2 * R, plane = kTile * pitch;
    float *const s0 = s_bloom, *const s1 = s_bloom + plane, *const s2 = s_bloom + 2 * plane;
    const auto [lane, wave, lx, ly] = tile_lane();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [x0, ty0] = tile_origin(tile, tiles_x, y0);
        // ---- the bright pass into LDS: a wavefront stages the rows it walks, 2 wave, 2 wave + 1 (+ 8 k)
        unsigned lit = 0;                       // bit k: a value staged for the k-th pair of rows is not +-0
#pragma unroll
        for (int k = 0; k < kTile / kTileRows; ++k) {
            bool some = false;
            for (int j = 0; j < 2; ++j) {
                const int sy = 2 * wave + j + k * kTileRows, gy = ty0 + sy;
                for (int sx = lane; sx < pitch; sx += 64) {
                    const int gx = x0 - R + sx;
                    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
                    if (gy < y1 && gx >= 0 && gx < W) {
                        const float *cp = src + ((size_t)gy * (size_t)W + (size_t)gx) * 3;
                        const float r = cp[0], g = cp[1], b = cp[2];
                        float m = r;
                        if (g > m) m = g;
                        if (b > m) m = b;
                        const float kk = m - A.threshold;
                        if (kk > 0.0f) {        // (a NaN m fails)
                            const float q = kk / m;
                            b0 = r * q; b1 = g * q; b2 = b * q;
                        }
                    }
                    const int at = sy * pitch + sx;
                    s0[at] = b0; s1[at] = b1; s2[at] = b2;
                    some = some || bloom_lit(b0) || bloom_lit(b1) || bloom_lit(b2);
                }
            }
            lit |= wave_any(some) ? 1u << k : 0u;
        }
        __syncthreads();
        // ---- the row taps of the tile's pixels, 32 x 8 at a time
#pragma unroll 1
        for (int k = 0; k < kTile / kTileRows; ++k) {
            const int row = ly + k * kTileRows;
            const int x = x0 + lx, y = ty0 + row;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            if ((lit >> k) & 1u)                // a scalar branch: this pair of rows has something bright in reach
                bloom_walk(s0, s1, s2, row * pitch + lx, 1, A, a0, a1, a2);
            if (x < W && y < y1) {
                float *op = hb + ((size_t)y * (size_t)W + (size_t)x) * 3;
                op[0] = a0; op[1] = a1; op[2] = a2;
            }
        }
        __syncthreads();                        // the next tile's staging overwrites what the taps read
    }
}

// crender_present_u8's cast (model_ops.hip): cvttss2si, then the low byte
__device__ inline unsigned char bloom_u8(float v)
{
    int iv = (int)0x80000000;
    if (v > -2147483904.0f && v < 2147483648.0f) iv = (int)v;
    return (unsigned char)((unsigned)iv & 0xFFu);
}

// Rules 5 and 6 on one channel.
__device__ inline float bloom_tone(float v, const BloomParams &A)
{
    float o = v;
    if (A.tone) {
        float a = v * A.exposure;
        a = a > 0.0f ? a : 0.0f;
        a = a * A.inv255;
        float L = a;
        if (A.reinhard) L = (a * (1.0f + a * A.iw2)) / (1.0f + a);
        if (A.gamma2) L = sqrtf(L);
        o = L * 255.0f;
    }
    return o > A.clamp ? A.clamp : o;           // (a NaN stays; a clamp of +inf is none)
}

template <bool U8>
__global__ __launch_bounds__(kThreads) void k_bloom_finish(const float *__restrict__ src, const float *__restrict__ hb,
                                                            BloomParams A, void *__restrict__ out, int W, int y0, int y1,
                                                            int tiles_x, int ntiles)
{
    extern __shared__ float s_bloom[];          // hb's r, g, b: [kTile + 2R][kTile] each; then a word per wavefront
    const int R = A.R, rows = kTile + 2 * R, plane = rows * kTile;
    float *const s0 = s_bloom, *const s1 = s_bloom + plane, *const s2 = s_bloom + 2 * plane;
    int *const s_lit = reinterpret_cast<int *>(s_bloom + 3 * plane);
    const auto [lane, wave, lx, ly] = tile_lane();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [x0, ty0] = tile_origin(tile, tiles_x, y0);
        // ---- stage hb of the tile and the R rows above and below it: a wavefront two rows at a time
        bool some = false;
        const int gx = x0 + lx;
        for (int sy = ly; sy < rows; sy += kTileRows) {
            const int gy = ty0 - R + sy;
            float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
            if (gy >= y0 && gy < y1 && gx < W) {
                const float *hp = hb + ((size_t)gy * (size_t)W + (size_t)gx) * 3;
                h0 = hp[0]; h1 = hp[1]; h2 = hp[2];
            }
            const int at = sy * kTile + lx;
            s0[at] = h0; s1[at] = h1; s2[at] = h2;
            some = some || bloom_lit(h0) || bloom_lit(h1) || bloom_lit(h2);
        }
        some = wave_any(some);
        if (lane == 0) s_lit[wave] = some ? 1 : 0;
        __syncthreads();
        int all = s_lit[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) all |= s_lit[w];
        const bool lit = wave_any(all != 0);    // a scalar branch: a dark tile walks nothing
        // ---- the column taps of the tile's pixels, 32 x 8 at a time; then rules 4 to 7
#pragma unroll 1
        for (int k = 0; k < kTile / kTileRows; ++k) {
            const int row = ly + k * kTileRows;
            const int x = x0 + lx, y = ty0 + row;
            float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
            if (lit) bloom_walk(s0, s1, s2, row * kTile + lx, kTile, A, g0, g1, g2);
            if (!(x < W && y < y1)) continue;
            const size_t pix = (size_t)y * (size_t)W + (size_t)x;
            const float *cp = src + pix * 3;
            float v0 = cp[0], v1 = cp[1], v2 = cp[2];
            const float t0 = A.intensity * g0, t1 = A.intensity * g1, t2 = A.intensity * g2;
            if (bloom_lit(t0) || bloom_lit(t1) || bloom_lit(t2)) {
                v0 = v0 + t0; v1 = v1 + t1; v2 = v2 + t2;
            }                                   // (otherwise the source's bits, a -0 and every NaN kept)
            v0 = bloom_tone(v0, A); v1 = bloom_tone(v1, A); v2 = bloom_tone(v2, A);
            const size_t opix = (size_t)(A.flip ? A.H - 1 - y : y) * (size_t)W + (size_t)x;
            if constexpr (U8) {
                unsigned char *op = reinterpret_cast<unsigned char *>(out) + opix * 3;
                op[0] = bloom_u8(v0); op[1] = bloom_u8(v1); op[2] = bloom_u8(v2);
            } else {
                float *op = reinterpret_cast<float *>(out) + opix * 3;
                op[0] = v0; op[1] = v1; op[2] = v2;
            }
        }
        __syncthreads();                        // the next tile's staging overwrites what the taps read
    }
}

}  // namespace

extern "C" {

int crender_bloom(const float *d_src, float threshold, const float *weights, int radius, float intensity, float exposure,
                  float inv_white2, float clamp, float *d_scratch, void *d_out, int H, int W, int y0, int y1, unsigned flags,
                  void *stream)
{
    const char *const E = "crender_bloom";
    if (int rc = frame_checks(E, 0, true, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (!d_src || !weights || !d_scratch || !d_out) return arg_error(E, "d_src, weights, d_scratch or d_out is NULL");
    if (radius < 1 || radius > CRENDER_BLOOM_MAX_RADIUS) return arg_error(E, "radius is not 1 .. 32");
    for (int k = 0; k <= radius; ++k)
        if (!isfinite(weights[k])) return arg_error(E, "a weight is not finite");
    if (!(threshold >= 0.0f)) return arg_error(E, "threshold is negative or NaN");
    if (!isfinite(intensity) || intensity < 0.0f) return arg_error(E, "intensity is not finite and 0 or above");
    if (!isfinite(exposure) || exposure < 0.0f) return arg_error(E, "exposure is not finite and 0 or above");
    if (!(inv_white2 >= 0.0f)) return arg_error(E, "inv_white2 is negative or NaN");
    if (clamp != clamp) return arg_error(E, "clamp is NaN");
    const unsigned known = CRENDER_BLOOM_U8 | CRENDER_BLOOM_FLIP | CRENDER_BLOOM_REINHARD | CRENDER_BLOOM_GAMMA2;
    if (flags & ~known) return arg_error(E, "unknown flag bits");
    if (d_out == (const void *)d_src || d_out == (const void *)d_scratch || d_scratch == d_src)
        return arg_error(E, "d_out, d_scratch and d_src are not three planes (the pass cannot run in place)");
    int tiles_x, tiles;
    if (int rc = tile_grid(E, W, y0, y1, tiles_x, tiles)) return rc;
    BloomParams A = {};
    A.threshold = threshold; A.intensity = intensity; A.exposure = exposure;
    A.inv255 = (float)(1.0 / 255.0); A.iw2 = inv_white2; A.clamp = clamp;
    A.R = radius; A.H = H;
    A.reinhard = (flags & CRENDER_BLOOM_REINHARD) ? 1 : 0;
    A.gamma2 = (flags & CRENDER_BLOOM_GAMMA2) ? 1 : 0;
    A.tone = (A.reinhard || A.gamma2 || exposure != 1.0f) ? 1 : 0;
    A.flip = (flags & CRENDER_BLOOM_FLIP) ? 1 : 0;
    for (int k = 0; k <= radius; ++k) A.w[k] = weights[k];
    const dim3 grid((unsigned)(tiles < kBloomMaxGrid ? tiles : kBloomMaxGrid));
    const size_t lds = (size_t)3 * kTile * (kTile + 2 * radius) * 4;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_bloom_rows, grid, dim3(kThreads), lds, st, d_src, A, d_scratch, W, y0, y1, tiles_x, tiles);
    CR_LAUNCH_CHECK("k_bloom_rows");
    if (flags & CRENDER_BLOOM_U8)
        hipLaunchKernelGGL(k_bloom_finish<true>, grid, dim3(kThreads), lds + (kThreads / 64) * 4, st, d_src,
                           (const float *)d_scratch, A, d_out, W, y0, y1, tiles_x, tiles);
    else
        hipLaunchKernelGGL(k_bloom_finish<false>, grid, dim3(kThreads), lds + (kThreads / 64) * 4, st, d_src,
                           (const float *)d_scratch, A, d_out, W, y0, y1, tiles_x, tiles);
    CR_LAUNCH_CHECK("k_bloom_finish");
    return CRENDER_OK;
}

}  // extern "C"
