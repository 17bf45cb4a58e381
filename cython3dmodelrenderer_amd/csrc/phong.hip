// phong.hip — per-pixel Blinn-Phong lighting as a deferred pass over the winner plane
// (include/crender_phong.h states the arithmetic; this file keeps its operation order).
//
// The shape of k_shadow_shade (shadow.hip): a pixel per work item, an 8 x 8 block of pixels per wavefront
// (a workgroup is four of them side by side: 32 x 8), a grid-stride loop over row blocks.  A wavefront whose
// 64 winners are all background leaves after its one load.  What is blended across the triangle is its own three
// unprojected corners: the surface point the pixel shows, in the camera's frame.
//
// The lights travel by value in the kernel's arguments; how many there are, which of them are directions and
// the number of squarings are the same for every lane, so the light loop and the squaring loop are scalar loops
// and the test of a light's kind is a scalar branch.  One light — the common case — has an instance without the
// loop frame.  Measured figures: README, "Phong illumination".
#include <math.h>

#include "common.h"
#include "../../include/crender_phong.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, winner_triangle, pass_grid, frame_checks

namespace {

// The lights and the coefficients of a call.
struct PhongLights {
    float v[CRENDER_PHONG_MAX_LIGHTS][5];    // x, y, z, kd, ks
    int n;
    unsigned directional;                    // bit j: light j is a direction
    float ambient;
    int squarings;                           // shininess_log2
    float spec[3];
    float clamp;
};

CR_DEV float len3(const float a[3])
{
    return sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
}

// The statements "Per light j" of crender_phong.h: d and sp of light j at the surface point p, seen along vu, with
// the normal n; after the `lit` selects.
CR_DEV void light_terms(const PhongLights &L, int j, const float p[3], const float vu[3], const float n[3], float &d,
                        float &sp)
{
    float lu[3] = {L.v[j][0], L.v[j][1], L.v[j][2]};
    if (!((L.directional >> j) & 1u)) {             // a scalar branch
        const float lv[3] = {lu[0] - p[0], lu[1] - p[1], lu[2] - p[2]};
        const float ll = len3(lv);
        lu[0] = lv[0] / ll;
        lu[1] = lv[1] / ll;
        lu[2] = lv[2] / ll;
    }
    d = guro_factor(Light{lu[0], lu[1], lu[2], 1}, n[0], n[1], n[2]);
    const float hv[3] = {lu[0] + vu[0], lu[1] + vu[1], lu[2] + vu[2]};
    const float hl = len3(hv);
    sp = guro_factor(Light{hv[0] / hl, hv[1] / hl, hv[2] / hl, 1}, n[0], n[1], n[2]);
    for (int k = 0; k < L.squarings; ++k) sp = sp * sp;
    const bool lit = d > 0.0f;
    d = lit ? d : 0.0f;
    sp = (lit && sp > 0.0f) ? sp : 0.0f;
}

template <bool ONE>
__global__ __launch_bounds__(kThreads) void k_phong_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                           int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                           const float *__restrict__ nb, PhongLights L,
                                                           float *__restrict__ cb, int W, int y0, int y1, int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!wave_any(px.covered)) continue;        // a scalar branch: the whole wavefront leaves
        if (!px.covered) continue;
        float raw[3][3];
        const TriXYZ X = winner_triangle(tri, px.t, P, raw);
        const float *A = raw[0], *B = raw[1], *Cc = raw[2];
        float b1, b2, b3;
        barycentric(X, px.x, px.y, b1, b2, b3);
        const float q1 = b1 / A[2], q2 = b2 / B[2], q3 = b3 / Cc[2];
        const float s = (q1 + q2) + q3;
        float p[3], v[3], vu[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            p[i] = ((A[i] * q1 + B[i] * q2) + Cc[i] * q3) / s;
            v[i] = -p[i];
        }
        const float vl = len3(v);
        vu[0] = v[0] / vl;
        vu[1] = v[1] / vl;
        vu[2] = v[2] / vl;
        const float *np_ = nb + px.pix * 3;
        const float n[3] = {np_[0], np_[1], np_[2]};
        float F = L.ambient, Ws = 0.0f;
        if (ONE) {
            float d, sp;
            light_terms(L, 0, p, vu, n, d, sp);
            F = F + L.v[0][3] * d;
            Ws = Ws + L.v[0][4] * sp;
        } else {
            for (int j = 0; j < L.n; ++j) {
                float d, sp;
                light_terms(L, j, p, vu, n, d, sp);
                F = F + L.v[j][3] * d;
                Ws = Ws + L.v[j][4] * sp;
            }
        }
        float *cp = cb + px.pix * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float o = cp[i] * F + Ws * L.spec[i];
            cp[i] = o > L.clamp ? L.clamp : o;
        }
    }
}

}  // namespace

extern "C" {

int crender_phong_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                        const float *P16, const float *d_normal, const float *lights5, int n_lights,
                        unsigned directional_mask, float ambient, int shininess_log2, const float *spec_color3,
                        float clamp, float *d_color, int H, int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_phong_shade";
    if (!d_winner || !P16 || !d_normal || !lights5 || !spec_color3 || !d_color)
        return arg_error(E, "d_winner, P16, d_normal, lights5, spec_color3 or d_color is NULL");
    if (int rc = frame_checks(E, T, d_tri, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (n_lights < 1 || n_lights > CRENDER_PHONG_MAX_LIGHTS) return arg_error(E, "n_lights is not 1 .. 4");
    if (directional_mask >> n_lights) return arg_error(E, "directional_mask has bits at or above n_lights");
    if (shininess_log2 < 0 || shininess_log2 > CRENDER_PHONG_MAX_SHININESS_LOG2)
        return arg_error(E, "shininess_log2 is not 0 .. 12");
    bool finite = isfinite(ambient) && isfinite(spec_color3[0]) && isfinite(spec_color3[1]) && isfinite(spec_color3[2]);
    bool negative = ambient < 0.0f;
    for (int j = 0; j < n_lights; ++j)
        for (int i = 0; i < 5; ++i) {
            finite = finite && isfinite(lights5[j * 5 + i]);
            negative = negative || (i >= 3 && lights5[j * 5 + i] < 0.0f);
        }
    if (!finite) return arg_error(E, "ambient, a light or spec_color3 is not finite");
    if (negative) return arg_error(E, "ambient, kd or ks is negative");
    if (clamp != clamp) return arg_error(E, "clamp is NaN");
    if (flags) return arg_error(E, "unknown flag bits");
    if (T == 0) return CRENDER_OK;
    PhongLights L{};
    for (int j = 0; j < n_lights; ++j)
        for (int i = 0; i < 5; ++i) L.v[j][i] = lights5[j * 5 + i];
    L.n = n_lights;
    L.directional = directional_mask;
    L.ambient = ambient;
    L.squarings = shininess_log2;
    L.spec[0] = spec_color3[0]; L.spec[1] = spec_color3[1]; L.spec[2] = spec_color3[2];
    L.clamp = clamp;
    // [one light: no loop frame]
    static constexpr decltype(&k_phong_shade<false>) kernels[2] = {k_phong_shade<false>, k_phong_shade<true>};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[n_lights == 1], G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner,
                       d_tri, T, d_pos_of, make_proj(P16, W, H), d_normal, L, d_color, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_phong_shade");
    return CRENDER_OK;
}

}  // extern "C"
