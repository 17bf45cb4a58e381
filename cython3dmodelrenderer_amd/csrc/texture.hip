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

namespace {

constexpr int kTexBlock = 8;         // pixels along each side of a wavefront's block

// The host's truncating float -> int32 conversion (cvttss2si): INT_MIN for a NaN and out of range.
// (Restated from model_ops.hip, whose text is fingerprinted.)
CR_DEV int host_f32_to_i32(float f)
{
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000;
}

CR_DEV const unsigned char *texel(const unsigned char *__restrict__ tex, int row, int colm, int tw)
{
    return tex + ((size_t)row * (size_t)tw + (size_t)colm) * 3;
}

template <bool PERSPECTIVE, bool BILINEAR, bool LIGHT>
__global__ __launch_bounds__(kThreads) void k_tex_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                         int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                         const float *__restrict__ uv,
                                                         const unsigned char *__restrict__ tex, int th, int tw,
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
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
        if (covered) {
            float a[3], b[3], c[3];
            const float *v = tri + t * 9;
            a[0] = v[0]; a[1] = v[1]; a[2] = v[2];
            b[0] = v[3]; b[1] = v[4]; b[2] = v[5];
            c[0] = v[6]; c[1] = v[7]; c[2] = v[8];
            const float za = a[2], zb = b[2], zc = c[2];
            project_vertex(P, a);
            project_vertex(P, b);
            project_vertex(P, c);
            const TriXYZ X{a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]};
            float b1, b2, b3;
            barycentric(X, x, y, b1, b2, b3);
            const float *w = uv + orig * 6;
            const float u0 = w[0], v0 = w[1], u1 = w[2], v1 = w[3], u2 = w[4], v2 = w[5];
            float tu, tv;
            if (PERSPECTIVE) {
                const float q1 = b1 / za, q2 = b2 / zb, q3 = b3 / zc;
                const float s = (q1 + q2) + q3;
                tu = ((u0 * q1 + u1 * q2) + u2 * q3) / s;
                tv = ((v0 * q1 + v1 * q2) + v2 * q3) / s;
            } else {
                tu = interp(u0, u1, u2, b1, b2, b3);
                tv = interp(v0, v1, v2, b1, b2, b3);
            }
            if (BILINEAR) {
                const float fx = tu * (float)tw - 0.5f, fy = (1.0f - tv) * (float)th - 0.5f;
                const float x0 = floorf(fx), yf0 = floorf(fy);
                const float ax = fx - x0, ay = fy - yf0;
                const int cl = clipi(host_f32_to_i32(x0), 0, tw - 1), cr = clipi(host_f32_to_i32(x0 + 1.0f), 0, tw - 1);
                const int rt = clipi(host_f32_to_i32(yf0), 0, th - 1), rbm = clipi(host_f32_to_i32(yf0 + 1.0f), 0, th - 1);
                const unsigned char *t00 = texel(tex, rt, cl, tw), *t01 = texel(tex, rt, cr, tw);
                const unsigned char *t10 = texel(tex, rbm, cl, tw), *t11 = texel(tex, rbm, cr, tw);
                const float wx = 1.0f - ax, wy = 1.0f - ay;
                c0 = ((float)t00[0] * wx + (float)t01[0] * ax) * wy + ((float)t10[0] * wx + (float)t11[0] * ax) * ay;
                c1 = ((float)t00[1] * wx + (float)t01[1] * ax) * wy + ((float)t10[1] * wx + (float)t11[1] * ax) * ay;
                c2 = ((float)t00[2] * wx + (float)t01[2] * ax) * wy + ((float)t10[2] * wx + (float)t11[2] * ax) * ay;
            } else {
                const int row = clipi(host_f32_to_i32((1.0f - tv) * (float)th), 0, th - 1);
                const int colm = clipi(host_f32_to_i32(tu * (float)tw), 0, tw - 1);
                const unsigned char *p = texel(tex, row, colm, tw);
                c0 = (float)p[0]; c1 = (float)p[1]; c2 = (float)p[2];
            }
        }
        if (LIGHT) {
            if (!inside) continue;
            float *cp = cb + pix * 3;
            const float *np_ = nb + pix * 3;
            if (!covered) { c0 = cp[0]; c1 = cp[1]; c2 = cp[2]; }
            const float f = guro_factor(L, np_[0], np_[1], np_[2]);
            cp[0] = c0 * f; cp[1] = c1 * f; cp[2] = c2 * f;
        } else if (covered) {
            float *cp = cb + pix * 3;
            cp[0] = c0; cp[1] = c1; cp[2] = c2;
        }
    }
}

template <bool PERSPECTIVE, bool BILINEAR>
void launch_tex(bool light, dim3 grid, hipStream_t st, const int32_t *win, const float *tri, int64_t T,
                const uint32_t *pos_of, const ProjConst &P, const float *uv, const unsigned char *tex, int th, int tw,
                const float *nb, const Light &L, float *cb, int W, int y0, int y1, int row_blocks)
{
    if (light)
        hipLaunchKernelGGL((k_tex_shade<PERSPECTIVE, BILINEAR, true>), grid, dim3(kThreads), 0, st, win, tri, T, pos_of,
                           P, uv, tex, th, tw, nb, L, cb, W, y0, y1, row_blocks);
    else
        hipLaunchKernelGGL((k_tex_shade<PERSPECTIVE, BILINEAR, false>), grid, dim3(kThreads), 0, st, win, tri, T, pos_of,
                           P, uv, tex, th, tw, nb, L, cb, W, y0, y1, row_blocks);
}

}  // namespace

extern "C" {

int crender_tex_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                      const float *P16, const float *d_uv, const unsigned char *d_texture, int th, int tw,
                      const float *d_normal, const float *light3, float *d_color, int H, int W, int y0, int y1,
                      unsigned flags, void *stream)
{
    if (!d_winner || !P16 || !d_texture || !d_color || T < 0 || (T > 0 && (!d_tri || !d_uv)) || th < 1 || tw < 1 ||
        H < 1 || W < 1 || y0 < 0 || y1 > H || y0 >= y1 || (light3 && !d_normal) || (d_normal && !light3) ||
        (flags & ~(unsigned)(CRENDER_TEX_PERSPECTIVE | CRENDER_TEX_BILINEAR)))
        return fail(CRENDER_EINVAL, "crender_tex_shade: bad argument");
    const bool light = light3 != nullptr;
    if (T == 0 && !light) return CRENDER_OK;
    const ProjConst P = make_proj(P16, W, H);
    const Light L = light ? Light{light3[0], light3[1], light3[2], 1} : Light{0.0f, 0.0f, 0.0f, 0};
    const int row_blocks = (y1 - y0 + kTexBlock - 1) / kTexBlock;
    const int across = kTexBlock * (kThreads / 64);
    const dim3 grid((unsigned)((W + across - 1) / across), (unsigned)(row_blocks < 65535 ? row_blocks : 65535));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool persp = flags & CRENDER_TEX_PERSPECTIVE, bilin = flags & CRENDER_TEX_BILINEAR;
    if (persp && bilin)
        launch_tex<true, true>(light, grid, st, d_winner, d_tri, T, d_pos_of, P, d_uv, d_texture, th, tw, d_normal, L,
                               d_color, W, y0, y1, row_blocks);
    else if (persp)
        launch_tex<true, false>(light, grid, st, d_winner, d_tri, T, d_pos_of, P, d_uv, d_texture, th, tw, d_normal, L,
                                d_color, W, y0, y1, row_blocks);
    else if (bilin)
        launch_tex<false, true>(light, grid, st, d_winner, d_tri, T, d_pos_of, P, d_uv, d_texture, th, tw, d_normal, L,
                                d_color, W, y0, y1, row_blocks);
    else
        launch_tex<false, false>(light, grid, st, d_winner, d_tri, T, d_pos_of, P, d_uv, d_texture, th, tw, d_normal,
                                 L, d_color, W, y0, y1, row_blocks);
    CR_LAUNCH_CHECK("k_tex_shade");
    return CRENDER_OK;
}

}  // extern "C"
