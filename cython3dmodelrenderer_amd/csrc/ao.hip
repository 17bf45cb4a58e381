// ao.hip — screen-space ambient occlusion as a deferred pass over the z, winner and normal planes
// (include/crender_ao.h states the arithmetic; this file keeps its operation order).
//
// The first NEIGHBOURHOOD pass: a covered pixel reads tens of view depths around it.  A workgroup owns a tile of
// kTile x kTile pixels and stages zv = P14 / (z - P10) of the tile plus a halo of radius_px on every side into LDS
// once: one division per staged pixel, not one per tap; unit-stride loads of d_z and d_winner along rows.  A staged
// pixel that is uncovered — off the frame, outside the strip, a winner outside [0, T) — gets a NaN: every
// comparison of `take` is then false, which is the contract's o_i = +0 without a second array.  (A covered pixel
// whose own zv is a NaN takes the same way through the same statements.)
//
// Geometry.  256 work items are 32 x 8 pixels; a wavefront is two rows of 32, and it walks the tile's 32 rows in
// four steps of 8.  ds_read_b32 is served in two lane groups, {0-31} and {32-63}, 32 banks of 4 bytes: a lane group
// is ONE row of 32 consecutive words, so a tap's read — every lane at its own base plus the same offset — is free of
// bank conflicts under any pitch, and the pitch is simply tile + 2 * radius_px.  The LDS is sized at launch:
// (32 + 2R)^2 words, 4.6 KB at R = 1, 9.2 KB at R = 8, 36.9 KB at R = 32 — four workgroups per CU at the largest.
// With the rotation a lane takes one of four quarter turns of the offset by its pixel's parity: neighbouring lanes
// then read different rows and may share a bank.
//
// The tap table and every constant travel by value in the kernel's arguments; the tap loop is a scalar loop.
// Measured figures: README, "Ambient occlusion".
#include <math.h>

#include "common.h"
#include "../../include/crender_ao.h"

using namespace crender_detail;

#include "winner_pass.h"     // gather_corners, the tile frame (kTile, TileLane, tile_origin), tile_grid, frame_checks

namespace {

constexpr int kMaxGrid = 2048;            // workgroups of a launch: 8 per CU; the kernel loops over the other tiles

// The taps and the constants of a call.
struct AoParams {
    int32_t tap[CRENDER_AO_MAX_TAPS];     // (dx & 0xFFFF) | dy << 16
    int n, R;
    float p10, p14, xs, ys, kx, ky;
    float r2, inv_r2, inv_n, min_cos, strength, floor_;
};

template <bool FACE, bool ROTATE>
__global__ __launch_bounds__(kThreads) void k_ao_shade(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                        const float *__restrict__ tri, int64_t T,
                                                        const uint32_t *__restrict__ pos_of,
                                                        const float *__restrict__ nb, AoParams A,
                                                        float *__restrict__ cb, int W, int y0, int y1, int tiles_x,
                                                        int ntiles)
{
    extern __shared__ float s_zv[];       // [kTile + 2R][kTile + 2R]
    const int R = A.R, pitch = kTile + 2 * R;
    const auto [lane, wave, lx, ly] = tile_lane();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [x0, ty0] = tile_origin(tile, tiles_x, y0);
        // ---- stage zv of the tile and its halo: a wavefront per row, 64 columns at a time
        for (int sy = wave; sy < pitch; sy += kThreads / 64) {
            const int gy = ty0 - R + sy;
            const bool row_in = gy >= y0 && gy < y1;
            for (int sx = lane; sx < pitch; sx += 64) {
                const int gx = x0 - R + sx;
                float zv = __builtin_nanf("");
                if (row_in && gx >= 0 && gx < W) {
                    const size_t pix = (size_t)gy * (size_t)W + (size_t)gx;
                    const int32_t w = win[pix];
                    const float z = zb[pix];            // (both loads in flight together: the address is good either way)
                    if (w >= 0 && w < T) zv = A.p14 / (z - A.p10);
                }
                s_zv[sy * pitch + sx] = zv;
            }
        }
        __syncthreads();
        // ---- the tile's pixels, 32 x 8 at a time
#pragma unroll 1
        for (int k = 0; k < kTile / kTileRows; ++k) {
            const int row = ly + k * kTileRows;
            const int x = x0 + lx, y = ty0 + row;
            const bool inside = x < W && y < y1;
            const size_t pix = (size_t)y * (size_t)W + (size_t)x;
            int64_t t = -1;
            if (inside) t = win[pix];
            bool covered = t >= 0 && t < T;
            if (FACE && covered && pos_of) {
                t = pos_of[t];
                covered = t < T;
            }
            if (!wave_any(covered)) continue;           // a scalar branch: the whole wavefront skips the taps
            if (!covered) continue;
            const int base = (row + R) * pitch + lx + R;
            const float fx = ((float)x - A.xs) * A.kx, fy = ((float)y - A.ys) * A.ky;
            const float pz = s_zv[base];
            const float px = fx * pz, py = fy * pz;
            float n0, n1, n2;
            if (FACE) {
                float a[3], b[3], c[3];
                gather_corners(tri, t, a, b, c);
                const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
                const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
                n0 = e1y * e2z - e1z * e2y;
                n1 = e1z * e2x - e1x * e2z;
                n2 = e1x * e2y - e1y * e2x;
                const float s = (n0 * px + n1 * py) + n2 * pz;
                if (s > 0.0f) { n0 = -n0; n1 = -n1; n2 = -n2; }
            } else {
                const float *np_ = nb + pix * 3;
                n0 = np_[0]; n1 = np_[1]; n2 = np_[2];
            }
            const float ln = sqrtf((n0 * n0 + n1 * n1) + n2 * n2) + 1e-6f;
            const float nu0 = n0 / ln, nu1 = n1 / ln, nu2 = n2 / ln;
            // the quarter turn of this pixel: (dx, dy) -> (a*dx + b*dy, c*dx + d*dy)
            int ra = 1, rb = 0, rc = 0, rd = 1;
            if (ROTATE) {
                const int r = (x & 1) | ((y & 1) << 1);
                ra = r == 0 ? 1 : (r == 3 ? -1 : 0);
                rb = r == 1 ? -1 : (r == 2 ? 1 : 0);
                rc = -rb;
                rd = ra;
            }
            float S = 0.0f;
            for (int i = 0; i < A.n; ++i) {             // a scalar loop: the table is the same for every lane
                const int32_t v = A.tap[i];
                const int tdx = (int)(int16_t)(v & 0xFFFF), tdy = v >> 16;
                const int dx = ROTATE ? ra * tdx + rb * tdy : tdx;
                const int dy = ROTATE ? rc * tdx + rd * tdy : tdy;
                const float qz = s_zv[base + dy * pitch + dx];
                const float qx = (((float)(x + dx) - A.xs) * A.kx) * qz;
                const float qy = (((float)(y + dy) - A.ys) * A.ky) * qz;
                const float Dx = qx - px, Dy = qy - py, Dz = qz - pz;
                const float dd = (Dx * Dx + Dy * Dy) + Dz * Dz;
                const float dn = (Dx * nu0 + Dy * nu1) + Dz * nu2;
                const float c = dn / sqrtf(dd);
                const float wgt = 1.0f - dd * A.inv_r2;
                const bool take = dd < A.r2 && c > A.min_cos;
                S = S + (take ? c * wgt : 0.0f);
            }
            if (!(S > 0.0f)) continue;
            float f = 1.0f - A.strength * (S * A.inv_n);
            f = f < A.floor_ ? A.floor_ : f;
            float *cp = cb + pix * 3;
            cp[0] = cp[0] * f; cp[1] = cp[1] * f; cp[2] = cp[2] * f;
        }
        __syncthreads();                                // the next tile's staging overwrites what the taps read
    }
}

}  // namespace

extern "C" {

int crender_ao_shade(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                     const float *P16, const float *d_normal, const int8_t *taps2, int n_taps, int radius_px,
                     float radius, float min_cos, float strength, float floor, float *d_color, int H, int W, int y0,
                     int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_ao_shade";
    if (!d_winner || !d_z || !P16 || !taps2 || !d_color) return arg_error(E, "d_winner, d_z, P16, taps2 or d_color is NULL");
    if (flags & ~(CRENDER_AO_ROTATE | CRENDER_AO_FACE_NORMALS)) return arg_error(E, "unknown flag bits");
    const bool face = (flags & CRENDER_AO_FACE_NORMALS) != 0, rotate = (flags & CRENDER_AO_ROTATE) != 0;
    if (!face && !d_normal) return arg_error(E, "d_normal is NULL without CRENDER_AO_FACE_NORMALS");
    if (int rc = frame_checks(E, T, !face || d_tri, H, W, "d_tri is NULL with CRENDER_AO_FACE_NORMALS and T > 0")) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (n_taps < 1 || n_taps > CRENDER_AO_MAX_TAPS) return arg_error(E, "n_taps is not 1 .. 64");
    if (radius_px < 1 || radius_px > CRENDER_AO_MAX_RADIUS_PX) return arg_error(E, "radius_px is not 1 .. 32");
    for (int i = 0; i < n_taps; ++i) {
        const int dx = taps2[2 * i], dy = taps2[2 * i + 1];
        if (dx > radius_px || dx < -radius_px || dy > radius_px || dy < -radius_px)
            return arg_error(E, "a tap reaches beyond radius_px");
        if (dx == 0 && dy == 0) return arg_error(E, "a tap is (0, 0)");
    }
    if (!isfinite(radius) || radius <= 0.0f) return arg_error(E, "radius is not finite and positive");
    if (!isfinite(min_cos) || !isfinite(strength) || !isfinite(floor))
        return arg_error(E, "min_cos, strength or floor is not finite");
    if (strength < 0.0f) return arg_error(E, "strength is negative");
    if (floor < 0.0f || floor > 1.0f) return arg_error(E, "floor is not 0 .. 1");
    if (int rc = projection_shape_check(E, P16)) return rc;
    if (T == 0) return CRENDER_OK;
    const ProjConst P = make_proj(P16, W, H);
    AoParams A{};
    for (int i = 0; i < n_taps; ++i)
        A.tap[i] = (int32_t)(((uint32_t)(int32_t)taps2[2 * i] & 0xFFFFu) | ((uint32_t)(int32_t)taps2[2 * i + 1] << 16));
    A.n = n_taps;
    A.R = radius_px;
    A.p10 = P16[10];
    A.p14 = P16[14];
    A.xs = P.xs;
    A.ys = P.ys;
    A.kx = (float)(1.0 / ((double)P.xs * (double)P16[0]));
    A.ky = (float)(1.0 / ((double)P.ys * (double)P16[5]));
    A.r2 = radius * radius;
    A.inv_r2 = (float)(1.0 / ((double)radius * (double)radius));
    A.inv_n = (float)(1.0 / (double)n_taps);
    A.min_cos = min_cos;
    A.strength = strength;
    A.floor_ = floor;
    int tiles_x, tiles;
    if (int rc = tile_grid(E, W, y0, y1, tiles_x, tiles)) return rc;
    static constexpr decltype(&k_ao_shade<false, false>) kernels[4] = {k_ao_shade<false, false>, k_ao_shade<false, true>,
                                                                        k_ao_shade<true, false>, k_ao_shade<true, true>};
    hipLaunchKernelGGL(kernels[(face ? 2 : 0) | (rotate ? 1 : 0)], dim3((unsigned)(tiles < kMaxGrid ? tiles : kMaxGrid)),
                       dim3(kThreads), tile_lds_bytes(radius_px), static_cast<hipStream_t>(stream), d_winner, d_z, d_tri, T,
                       d_pos_of, d_normal, A, d_color, W, y0, y1, tiles_x, tiles);
    CR_LAUNCH_CHECK("k_ao_shade");
    return CRENDER_OK;
}

}  // extern "C"
