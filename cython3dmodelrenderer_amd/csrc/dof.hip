// dof.hip — depth of field as a gather blur by the circle of confusion over the z plane
// (include/crender_dof.h states the arithmetic; this file keeps its operation order).
#include <math.h>

#include "common.h"
#include "../../include/crender_dof.h"

using namespace crender_detail;

#include "winner_pass.h"     // the tile frame (kTile, TileLane, tile_origin), tile_grid, frame_checks, rows_check

// ---- depth of field (crender_dof_blur) ----
// The frame through a lens: a gather blur by the circle of confusion the z plane gives.  A neighbourhood pass of the
// shape of k_ao_shade (ao.hip): a workgroup of 256 per tile of kTile x kTile pixels, looping over tiles, stages the tile
// plus a halo of max_radius on every side into LDS once, a wavefront per staged row with unit-stride loads — but FIVE words a
// pixel: the signed circle of confusion s, the reciprocal of its footprint ia (the one division, per STAGED pixel, so
// that no tap divides), and the three colours, in five planes of (32 + 2 R)^2 words: 23.1 KB at R = 1, 46.1 KB at R = 8,
// 62.7 KB at R = 12, which is where the 64 KB end and why the radius does.  A staged pixel off the frame or outside the
// strip gets s = NaN: every tap's `k > 0` then fails, and it contributes nowhere.
//
// Geometry.  k_ao_shade's: 256 work items are 32 x 8 pixels, a wavefront two rows of 32, so a lane group of a
// ds_read_b32 is ONE row of 32 consecutive words and a tap's reads — every lane at its own base plus the same offset, in
// each plane — are free of bank conflicts under any pitch.
//
// Work.  A pixel walks (2 Rt + 1)^2 taps, dy outer and dx inner, both ascending: the contract's order, since the sums
// are float32.  Rt = ceil(the largest c the workgroup staged), reduced while staging (a wavefront's own maximum by DPP,
// one LDS word per wavefront): a tap beyond it has k <= 0 for every pixel of the tile (r + 1 <= Rt + 1 <= dist, both
// roundings monotone), so the bits are the full window's.  A tile in focus with nothing blurred around it has Rt = 0 and
// copies its pixels.  A tap reads s and ia of q (two ds_read_b32) and dist from a table of 13 x 13 words (a
// wave-uniform address: a broadcast) and decides; the taps go four at a time, so that eight reads are in flight, and
// only if a lane of the wavefront takes one of the four (a scalar branch) their colours are read, twelve reads in
// flight.  The sums are made in the taps' own order.  No tap divides or takes a root.

namespace {

constexpr int kDofMaxGrid = 2048;            // workgroups of a launch: 8 per CU; the kernel loops over the other tiles
constexpr int kDofSide = CRENDER_DOF_MAX_RADIUS + 1;      // the table of dist is [kDofSide][kDofSide], by |dy| and |dx|
constexpr int kDofMore = kThreads / 64 + kDofSide * kDofSide;    // the words of LDS after the five planes

// The constants of a call.
struct DofParams {
    float p10, p14, focus, band, aperture, Rf, pi;
    int R;
};

__global__ __launch_bounds__(kThreads) void k_dof_blur(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                        int64_t T, const float *__restrict__ cb, DofParams A,
                                                        float *__restrict__ ob, int W, int y0, int y1, int tiles_x,
                                                        int ntiles)
{
    extern __shared__ float s_dof[];            // s, ia, r, g, b: [kTile + 2R][kTile + 2R] each; then s_top, s_dist
    const int R = A.R, pitch = kTile + 2 * R, plane = pitch * pitch;
    float *const s_s = s_dof, *const s_ia = s_dof + plane;
    float *const s_c0 = s_dof + 2 * plane, *const s_c1 = s_dof + 3 * plane, *const s_c2 = s_dof + 4 * plane;
    int *const s_top = reinterpret_cast<int *>(s_dof + 5 * plane);      // per wavefront: the bits of its largest c
    float *const s_dist = s_dof + 5 * plane + kThreads / 64;
    const auto [lane, wave, lx, ly] = tile_lane();
    if ((int)threadIdx.x < kDofSide * kDofSide) {
        const int i = (int)threadIdx.x / kDofSide, j = (int)threadIdx.x - i * kDofSide;
        s_dist[threadIdx.x] = sqrtf((float)(i * i + j * j));
    }                                           // (read after the first tile's barrier)
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [x0, ty0] = tile_origin(tile, tiles_x, y0);
        // ---- stage s, ia and the colours of the tile and its halo: a wavefront per row (pitch <= 56 columns)
        int top = 0;                            // a non-NaN c is >= +0: its bits order as ints
        for (int sy = wave; sy < pitch; sy += kThreads / 64) {
            const int gy = ty0 - R + sy;
            const bool row_in = gy >= y0 && gy < y1;
            for (int sx = lane; sx < pitch; sx += 64) {
                const int gx = x0 - R + sx;
                float s = __builtin_nanf(""), c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
                if (row_in && gx >= 0 && gx < W) {
                    const size_t pix = (size_t)gy * (size_t)W + (size_t)gx;
                    const int32_t w = win[pix];
                    const float z = zb[pix];
                    const float *cp = cb + pix * 3;
                    c0 = cp[0]; c1 = cp[1]; c2 = cp[2];
                    s = A.aperture;
                    if (w >= 0 && w < T) {
                        const float zv = A.p14 / (z - A.p10);
                        float d = zv - A.focus;
                        d = d > A.band ? d - A.band : (d < -A.band ? d + A.band : 0.0f);
                        s = A.aperture * (d / zv);
                    }
                    s = s > A.Rf ? A.Rf : (s < -A.Rf ? -A.Rf : s);
                }
                const int at = sy * pitch + sx;
                s_s[at] = s;
                s_ia[at] = 1.0f / (1.0f + A.pi * (s * s));
                s_c0[at] = c0; s_c1[at] = c1; s_c2[at] = c2;
                const float c = fabsf(s);
                const int bits = c == c ? __float_as_int(c) : 0;
                top = bits > top ? bits : top;
            }
        }
        top = wave_reduce<true>(top);
        if (lane == 0) s_top[wave] = top;
        __syncthreads();
        int all = s_top[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) all = s_top[w] > all ? s_top[w] : all;
        // the reach of this tile's taps: wave-uniform, 0 .. R (every c is clamped to Rf = R)
        int Rt = __builtin_amdgcn_readfirstlane((int)ceilf(__int_as_float(all)));
        Rt = Rt < R ? Rt : R;                   // (it is: kept as a guard of the LDS offsets)
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
            if (Rt == 0) {                              // a scalar branch: nothing around here is blurred
                if (inside) { op[0] = own0; op[1] = own1; op[2] = own2; }
                continue;
            }
            const float sp = s_s[base], iap = s_ia[base], cp = fabsf(sp);
            float Sw = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f;
            bool other = false;                         // a tap other than the centre was taken
            for (int dy = -Rt; dy <= Rt; ++dy) {
                const float *dist_row = s_dist + (dy < 0 ? -dy : dy) * kDofSide;
                const int row_at = base + dy * pitch;
                // four taps at a time: their reads of s and ia are in flight together (a tap's decision waits for its
                // reads: one tap at a time the loop is bound by the latency of the LDS), then the colours of the four if
                // a lane takes any of them, then the sums in the taps' own order.  (A word past the window's end is still
                // inside the allocation, the table follows the planes, and is not used.)
                for (int dx0 = -Rt; dx0 <= Rt; dx0 += 4) {
                    float kk[4], aa[4];
                    bool take[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int dx = dx0 + j, at = row_at + dx;
                        const float sq = s_s[at], iaq = s_ia[at];
                        const int adx = dx < 0 ? -dx : dx;
                        const float dist = dist_row[adx < kDofSide ? adx : kDofSide - 1];
                        const float cq = fabsf(sq);
                        const bool mine = sq > sp && cp < cq;   // q lies behind p and is blurred more: p's own radius
                        const float r = mine ? cp : cq;
                        aa[j] = mine ? iap : iaq;
                        kk[j] = (r + 1.0f) - dist;
                        take[j] = inside && dx <= Rt && kk[j] > 0.0f;       // (every NaN fails)
                    }
                    if (!wave_any(take[0] || take[1] || take[2] || take[3])) continue;    // a scalar branch: nobody reads the colours
                    float q0[4], q1[4], q2[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int at = row_at + dx0 + j;
                        q0[j] = s_c0[at]; q1[j] = s_c1[at]; q2[j] = s_c2[at];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (take[j]) {
                            const float w = (kk[j] < 1.0f ? kk[j] : 1.0f) * aa[j];
                            Sw = Sw + w;
                            S0 = S0 + w * q0[j];
                            S1 = S1 + w * q1[j];
                            S2 = S2 + w * q2[j];
                            other = other || ((dx0 + j) | dy) != 0;
                        }
                    }
                }
            }
            if (!inside) continue;
            if (!other || !(Sw > 0.0f)) {
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

int crender_dof_blur(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                     const float *P16, const float *d_color, float focus, float band, float aperture, int max_radius,
                     float *d_out, int H, int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_dof_blur";
    (void)d_tri;
    (void)d_pos_of;
    if (!d_winner || !d_z || !P16 || !d_color || !d_out) return arg_error(E, "d_winner, d_z, P16, d_color or d_out is NULL");
    if (int rc = frame_checks(E, T, true, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags) return arg_error(E, "unknown flag bits");
    if (d_out == d_color) return arg_error(E, "d_out is d_color (the pass cannot run in place)");
    if (int rc = projection_shape_check(E, P16)) return rc;
    if (!isfinite(focus) || !(focus > 0.0f)) return arg_error(E, "focus is not finite and positive");
    if (!isfinite(band) || band < 0.0f) return arg_error(E, "band is not finite and 0 or above");
    if (!isfinite(aperture) || aperture < 0.0f) return arg_error(E, "aperture is not finite and 0 or above");
    if (max_radius < 1 || max_radius > CRENDER_DOF_MAX_RADIUS) return arg_error(E, "max_radius is not 1 .. 12");
    int tiles_x, tiles;
    if (int rc = tile_grid(E, W, y0, y1, tiles_x, tiles)) return rc;
    const DofParams A = {P16[10], P16[14], focus, band, aperture, (float)max_radius, 3.14159265358979323846f, max_radius};
    // (T == 0: every pixel is background, s = aperture)
    hipLaunchKernelGGL(k_dof_blur, dim3((unsigned)(tiles < kDofMaxGrid ? tiles : kDofMaxGrid)), dim3(kThreads),
                       tile_lds_bytes(max_radius) * 5 + kDofMore * 4, static_cast<hipStream_t>(stream), d_winner, d_z, T,
                       d_color, A, d_out, W, y0, y1, tiles_x, tiles);
    CR_LAUNCH_CHECK("k_dof_blur");
    return CRENDER_OK;
}

}  // extern "C"
