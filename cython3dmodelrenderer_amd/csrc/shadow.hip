// shadow.hip — shadow mapping as a deferred pass over the winner plane
// (include/crender_shadow.h states the arithmetic; this file keeps its operation order).
//
// The shape of k_tex_shade (texture.hip): a pixel per work item, an 8 x 8 block of pixels per wavefront
// (a workgroup is four of them side by side: 32 x 8), a grid-stride loop over row blocks.  The "texture"
// is the z plane of a second frame, the light's, and what is blended across the triangle is its three
// light-frame corners (36 B per winner, gathered like the uv).  A wavefront whose 64 winners are all
// background leaves after its one load.
//
// The K x K taps are plain gathers with constant trip counts (the kernel is instantiated on K and on
// whether the light's winner plane is given): neighbouring pixels land on neighbouring texels, so the
// 64 lanes of a tap touch a few cache lines of the map.  Measured figures: README, "Shadow mapping".
#include <math.h>

#include "common.h"
#include "../../include/crender_shadow.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, winner_triangle, host_f32_to_i32, pass_grid, frame_checks

namespace {

// What the kernel needs of the light's frame.
struct ShadowMap {
    ProjConst P;                     // the light's projection, as make_proj(PL16, Wl, Hl)
    const float *z;                  // [Hl][Wl]
    const int32_t *winner;           // [Hl][Wl], read only by the WINNER instances
    int h, w;
    float bias, ambient;
};

template <int K, bool WINNER>
__global__ __launch_bounds__(kThreads) void k_shadow_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                            int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                            const float *__restrict__ ltri, ShadowMap M,
                                                            float *__restrict__ cb, int W, int y0, int y1, int row_blocks)
{
    constexpr int R = (K - 1) / 2;
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!wave_any(px.covered)) continue;        // a scalar branch: the whole wavefront leaves
        if (!px.covered) continue;
        const int64_t orig = px.orig;               // the winner in the caller's order: ltri, the light's winners
        float raw[3][3];
        const TriXYZ X = winner_triangle(tri, px.t, P, raw);
        float b1, b2, b3;
        barycentric(X, px.x, px.y, b1, b2, b3);
        const float q1 = b1 / raw[0][2], q2 = b2 / raw[1][2], q3 = b3 / raw[2][2];
        const float s = (q1 + q2) + q3;
        const float *l = ltri + orig * 9;
        float p[3];
        p[0] = ((l[0] * q1 + l[3] * q2) + l[6] * q3) / s;
        p[1] = ((l[1] * q1 + l[4] * q2) + l[7] * q3) / s;
        p[2] = ((l[2] * q1 + l[5] * q2) + l[8] * q3) / s;
        if (!(p[2] > 0.0f)) continue;               // behind the light, or NaN: every tap is lit
        project_vertex(M.P, p);
        // The tap sums stay in int32: the conversion's largest value is 2^31 - 128, so only a centre near INT_MIN
        // could overflow, and a centre three texels or more before the map has every tap outside it wherever it is.
        const int cx = max(host_f32_to_i32(floorf(p[0] + 0.5f)), -(R + 1));
        const int cy = max(host_f32_to_i32(floorf(p[1] + 0.5f)), -(R + 1));
        const float depth = p[2] - M.bias;
        // Every tap loads — a tap outside the map from the first texel of a row inside it — so that the K * K loads
        // are independent of the tests and issue back to back (measured against a branch per tap: README).
        int n = 0;
#pragma unroll
        for (int j = -R; j <= R; ++j) {
            const int row = cy + j;
            const bool row_in = (unsigned)row < (unsigned)M.h;
            const size_t row_at = row_in ? (size_t)row * (size_t)M.w : 0;
#pragma unroll
            for (int i = -R; i <= R; ++i) {
                const int colm = cx + i;
                const bool in = row_in && (unsigned)colm < (unsigned)M.w;
                const size_t at = row_at + (in ? (size_t)colm : 0);
                bool lit = !in || !(depth > M.z[at]);
                if (WINNER) lit = lit || (int64_t)M.winner[at] == orig;
                n += lit ? 1 : 0;
            }
        }
        if (n == K * K) continue;                   // lit: the pixel keeps its bits
        const float frac = (float)n / (float)(K * K);
        const float om = 1.0f - M.ambient;
        const float m = om * frac;
        const float f = M.ambient + m;
        float *cp = cb + px.pix * 3;
        cp[0] = cp[0] * f;
        cp[1] = cp[1] * f;
        cp[2] = cp[2] * f;
    }
}

}  // namespace

extern "C" {

int crender_shadow_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                         const float *P16, const float *d_ltri, const float *PL16, const float *d_lz,
                         const int32_t *d_lwinner, int Hl, int Wl, float bias, float ambient, int pcf, float *d_color,
                         int H, int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_shadow_shade";
    if (!d_winner || !P16 || !PL16 || !d_lz || !d_color) return arg_error(E, "d_winner, P16, PL16, d_lz or d_color is NULL");
    if (int rc = frame_checks(E, T, d_tri && d_ltri, H, W, "d_tri or d_ltri is NULL with T > 0")) return rc;
    if (Hl < 1 || Wl < 1) return arg_error(E, "Hl or Wl is below 1");
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (pcf != 1 && pcf != 3 && pcf != 5) return arg_error(E, "pcf is not 1, 3 or 5");
    if (!(ambient >= 0.0f && ambient <= 1.0f)) return arg_error(E, "ambient outside [0, 1] or NaN");
    if (!isfinite(bias)) return arg_error(E, "bias is not finite");
    if (flags) return arg_error(E, "unknown flag bits");
    if (T == 0) return CRENDER_OK;
    const ShadowMap M{make_proj(PL16, Wl, Hl), d_lz, d_lwinner, Hl, Wl, bias, ambient};
    // [pcf / 2][the light's winner plane given]
    static constexpr decltype(&k_shadow_shade<1, false>) kernels[3][2] = {
        {k_shadow_shade<1, false>, k_shadow_shade<1, true>},
        {k_shadow_shade<3, false>, k_shadow_shade<3, true>},
        {k_shadow_shade<5, false>, k_shadow_shade<5, true>}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[pcf / 2][d_lwinner != nullptr], G.grid, dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_winner, d_tri, T, d_pos_of, make_proj(P16, W, H), d_ltri, M,
                       d_color, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_shadow_shade");
    return CRENDER_OK;
}

}  // extern "C"
