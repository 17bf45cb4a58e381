// texture.hip — per-pixel texture mapping as a deferred pass over the winner plane
// (include/crender_tex.h states the arithmetic; this file keeps its operation order).
//
// A pixel per work item, an 8 x 8 block of pixels per wavefront (a workgroup is four of them side by
// side: 32 x 8), so that the lanes of a wavefront share winners and texels: their gathers of the
// triangle (36 B), its uv (24 B) and the texels land on a few cache lines, and the colour rows are
// 96 contiguous bytes per 8 lanes.  A wavefront whose 64 winners are all background, with no light to
// apply, leaves after its one load.
//
// Every covered pixel projects its winner's three vertices again.  De-duplicating winners within a
// wavefront was weighed and not built: the wavefront issues one instruction for all 64 lanes whether
// they hold one triangle or sixty-four, so the dozen divisions are paid once per wavefront either way,
// and lanes that share a winner read the same addresses, which the memory pipeline merges.  Only handing
// the distinct winners' vertices out to different lanes and passing the results through LDS would save
// arithmetic.  Measured (README, "Per-pixel texture mapping"): T-Rex 4096^2 without a light 47 us, i.e.
// 2.5 TB/s of plane bytes; with the light 127 us, 4.9 TB/s, against 5.6 TB/s for the illumination pass.
#include "common.h"
#include "../../include/crender_tex.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, winner_triangle, bilinear, store_shaded, pass_grid

namespace {

template <bool PERSPECTIVE, bool BILINEAR, bool LIGHT>
__global__ __launch_bounds__(kThreads) void k_tex_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                         int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                         const float *__restrict__ uv,
                                                         const unsigned char *__restrict__ tex, int th, int tw,
                                                         const float *__restrict__ nb, Light L,
                                                         float *__restrict__ cb, int W, int y0, int y1, int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!LIGHT && !wave_any(px.covered)) continue;
        float col[3] = {0.0f, 0.0f, 0.0f};
        if (px.covered) {
            float raw[3][3];
            const TriXYZ X = winner_triangle(tri, px.t, P, raw);
            float b1, b2, b3;
            barycentric(X, px.x, px.y, b1, b2, b3);
            const float *w = uv + px.orig * 6;
            const float u0 = w[0], v0 = w[1], u1 = w[2], v1 = w[3], u2 = w[4], v2 = w[5];
            float tu, tv;
            if (PERSPECTIVE) {
                const float q1 = b1 / raw[0][2], q2 = b2 / raw[1][2], q3 = b3 / raw[2][2];
                const float s = (q1 + q2) + q3;
                tu = ((u0 * q1 + u1 * q2) + u2 * q3) / s;
                tv = ((v0 * q1 + v1 * q2) + v2 * q3) / s;
            } else {
                tu = interp(u0, u1, u2, b1, b2, b3);
                tv = interp(v0, v1, v2, b1, b2, b3);
            }
            if (BILINEAR) {
                bilinear(tex, th, tw, tu, tv, col);
            } else {
                const int row = clipi(host_f32_to_i32((1.0f - tv) * (float)th), 0, th - 1);
                const int colm = clipi(host_f32_to_i32(tu * (float)tw), 0, tw - 1);
                const unsigned char *p = texel(tex, row, colm, tw);
                col[0] = (float)p[0]; col[1] = (float)p[1]; col[2] = (float)p[2];
            }
        }
        store_shaded<LIGHT>(px, col, nb, L, cb);
    }
}

}  // namespace

extern "C" {

int crender_tex_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                      const float *P16, const float *d_uv, const unsigned char *d_texture, int th, int tw,
                      const float *d_normal, const float *light3, float *d_color, int H, int W, int y0, int y1,
                      unsigned flags, void *stream)
{
    if (!frame_args_ok(d_winner, P16, d_color, T, d_tri, H, W, y0, y1) || !d_texture || (T > 0 && !d_uv) || th < 1 ||
        tw < 1 || !light_args_ok(light3, d_normal) ||
        (flags & ~(unsigned)(CRENDER_TEX_PERSPECTIVE | CRENDER_TEX_BILINEAR)))
        return fail(CRENDER_EINVAL, "crender_tex_shade: bad argument");
    const bool light = light3 != nullptr;
    if (T == 0 && !light) return CRENDER_OK;
    const bool persp = flags & CRENDER_TEX_PERSPECTIVE, bilin = flags & CRENDER_TEX_BILINEAR;
    // [perspective][bilinear][light]
    static constexpr decltype(&k_tex_shade<false, false, false>) kernels[2][2][2] = {
        {{k_tex_shade<false, false, false>, k_tex_shade<false, false, true>},
         {k_tex_shade<false, true, false>, k_tex_shade<false, true, true>}},
        {{k_tex_shade<true, false, false>, k_tex_shade<true, false, true>},
         {k_tex_shade<true, true, false>, k_tex_shade<true, true, true>}}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[persp][bilin][light], G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       d_winner, d_tri, T, d_pos_of, make_proj(P16, W, H), d_uv, d_texture, th, tw, d_normal,
                       pass_light(light3), d_color, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_tex_shade");
    return CRENDER_OK;
}

}  // extern "C"
