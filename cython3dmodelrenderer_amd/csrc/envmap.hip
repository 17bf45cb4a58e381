// envmap.hip — environment mapping: cube-map reflections and a skybox as a deferred pass over the winner plane
// (include/crender_env.h states the arithmetic; this file keeps its operation order).
#include <math.h>

#include "common.h"
#include "../../include/crender_env.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, winner_triangle, the texel fetches, pass_grid, frame_checks

// ---- environment mapping (crender_env_shade) ----
// A deferred pass that looks a direction up in a cube map: for a covered pixel the direction in which its surface mirrors
// the eye, for the others the pixel's own view ray.  The shape of k_phong_shade (phong.hip): a pixel per work item, an
// 8 x 8 block of pixels per wavefront, a grid-stride loop over row blocks; without the background a wavefront whose 64
// winners are all background leaves after its one load.  A covered pixel projects its winner and blends the triangle's
// own unprojected corners with the rasterizer's barycentrics, as that kernel does; the mirrored direction is not
// normalised, since the face and the two quotients of a direction do not depend on its length.  The orientation, the tint
// and the coefficients travel by value in the kernel's arguments.  The face of a direction comes from a chain of selects
// over its three components: a table indexed per lane would live in scratch.  Two levels of a chain are two face arrays
// the host picked; both samples' texel loads are independent of either blend, so the second does not wait for the first.

namespace {

// The operands of a call, by value.
struct EnvCall {
    float M[9];                          // the orientation, row-major
    float tint[3];
    float reflectivity, f0, one_minus_f0, gain;
    float frac;                          // the weight of the second level
    float xs, ys, kx, ky;                // crender_ao.h's host constants: a background pixel's ray
    int S0, S1;
};

// The face of direction d, its sc and tc and the major magnitude: the Face statement.
CR_DEV int env_face(const float d[3], float &sc, float &tc, float &ma)
{
    const float a0 = fabsf(d[0]), a1 = fabsf(d[1]), a2 = fabsf(d[2]);
    const bool X = a0 >= a1 && a0 >= a2;
    const bool Y = !X && a1 >= a2;
    ma = X ? a0 : (Y ? a1 : a2);
    const float dm = X ? d[0] : (Y ? d[1] : d[2]);
    const bool neg = dm < 0.0f;
    sc = X ? (neg ? d[2] : -d[2]) : (Y ? d[0] : (neg ? -d[0] : d[0]));
    tc = X ? d[1] : (Y ? (neg ? d[2] : -d[2]) : d[1]);
    return (X ? 0 : (Y ? 2 : 4)) + (neg ? 1 : 0);
}

template <bool REFLECT, bool BACKGROUND, bool TWO>
__global__ __launch_bounds__(kThreads) void k_env_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                         int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                         const float *__restrict__ nb,
                                                         const unsigned char *__restrict__ faces0,
                                                         const unsigned char *__restrict__ faces1, EnvCall E,
                                                         float *__restrict__ cb, int W, int y0, int y1, int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!BACKGROUND) {
            if (!wave_any(px.covered)) continue;    // a scalar branch: the whole wavefront leaves
            if (!px.covered) continue;
        } else {
            if (!px.inside) continue;
            if (!REFLECT && px.covered) continue;
        }
        const bool mirror = REFLECT && px.covered;
        float r[3], w = 0.0f;
        bool ok = true;
        if (mirror) {
            float raw[3][3];
            const TriXYZ X = winner_triangle(tri, px.t, P, raw);
            const float *A = raw[0], *B = raw[1], *Cc = raw[2];
            float b1, b2, b3;
            barycentric(X, px.x, px.y, b1, b2, b3);
            const float q1 = b1 / A[2], q2 = b2 / B[2], q3 = b3 / Cc[2];
            const float s = (q1 + q2) + q3;
            float p[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) p[i] = ((A[i] * q1 + B[i] * q2) + Cc[i] * q3) / s;
            const float *np_ = nb + px.pix * 3;
            const float n[3] = {np_[0], np_[1], np_[2]};
            const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
            const float ni = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2];
            const float k = (2.0f * ni) / nn;
#pragma unroll
            for (int i = 0; i < 3; ++i) r[i] = p[i] - k * n[i];
            const float pp = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
            const float c = fabsf(ni) / (sqrtf(nn) * sqrtf(pp));
            float m = 1.0f - c;
            m = m < 0.0f ? 0.0f : m;
            m = m > 1.0f ? 1.0f : m;
            ok = m == m;
            const float m2 = m * m;
            const float m5 = (m2 * m2) * m;
            w = E.reflectivity * (E.f0 + E.one_minus_f0 * m5);
        } else {
            r[0] = ((float)px.x - E.xs) * E.kx;
            r[1] = ((float)px.y - E.ys) * E.ky;
            r[2] = 1.0f;
        }
        float d[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = (E.M[3 * i] * r[0] + E.M[3 * i + 1] * r[1]) + E.M[3 * i + 2] * r[2];
        float sc, tc, ma;
        const int face = env_face(d, sc, tc, ma);
        if (!(ok && ma > 0.0f && ma < INFINITY)) continue;
        const float tu = (sc / ma + 1.0f) * 0.5f, tv = (1.0f - tc / ma) * 0.5f;
        float e[3];
        bilinear(faces0 + (size_t)face * ((size_t)E.S0 * (size_t)E.S0 * 3), E.S0, E.S0, tu, tv, e);
        if (TWO) {
            float up[3];
            bilinear(faces1 + (size_t)face * ((size_t)E.S1 * (size_t)E.S1 * 3), E.S1, E.S1, tu, tv, up);
            const float g = 1.0f - E.frac;
#pragma unroll
            for (int j = 0; j < 3; ++j) e[j] = e[j] * g + up[j] * E.frac;
        }
        float *cp = cb + px.pix * 3;
        if (mirror) {
            const float ow = 1.0f - w;
#pragma unroll
            for (int j = 0; j < 3; ++j) cp[j] = cp[j] * ow + (e[j] * E.tint[j]) * w;
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) cp[j] = e[j] * E.gain;
        }
    }
}

}  // namespace

extern "C" {

int crender_env_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of, const float *P16,
                      const float *d_normal, const uint8_t *d_faces0, int S0, const uint8_t *d_faces1, int S1,
                      float level_frac, const float *M9, float reflectivity, float f0, const float *tint3,
                      float background_gain, float *d_color, int H, int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_env_shade";
    bool reflect = flags & CRENDER_ENV_REFLECT;
    const bool background = flags & CRENDER_ENV_BACKGROUND;
    if (!d_winner || !P16 || !d_faces0 || !M9 || !tint3 || !d_color)
        return arg_error(E, "d_winner, P16, d_faces0, M9, tint3 or d_color is NULL");
    if (reflect && !d_normal) return arg_error(E, "d_normal is NULL with CRENDER_ENV_REFLECT");
    if (int rc = frame_checks(E, T, d_tri, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (S0 < 1 || S0 > CRENDER_ENV_MAX_SIDE) return arg_error(E, "S0 is not 1 .. 8192");
    if (S1 < 0 || S1 > CRENDER_ENV_MAX_SIDE) return arg_error(E, "S1 is not 0 .. 8192");
    const bool two = d_faces1 != nullptr;
    if (two ? !(S1 >= 1 && level_frac > 0.0f && level_frac < 1.0f) : !(S1 == 0 && level_frac == 0.0f))
        return arg_error(E, "d_faces1, S1 and level_frac are neither all given (0 < level_frac < 1) nor all absent");
    bool finite = isfinite(background_gain) && isfinite(tint3[0]) && isfinite(tint3[1]) && isfinite(tint3[2]);
    for (int i = 0; i < 9; ++i) finite = finite && isfinite(M9[i]);
    if (!finite) return arg_error(E, "M9, tint3 or background_gain is not finite");
    if (!(reflectivity >= 0.0f && reflectivity <= 1.0f) || !(f0 >= 0.0f && f0 <= 1.0f))
        return arg_error(E, "reflectivity or f0 is not 0 .. 1");
    if (background_gain < 0.0f) return arg_error(E, "background_gain is negative");
    if (background)
        for (int i : {0, 5})
            if (!isfinite(P16[i]) || P16[i] == 0.0f)
                return arg_error(E, "P16 is not of crender_projection_matrix's shape (entry 0 or 5 is 0 or not finite)");
    if (flags & ~(unsigned)(CRENDER_ENV_REFLECT | CRENDER_ENV_BACKGROUND)) return arg_error(E, "unknown flag bits");
    if (!reflect && !background) return arg_error(E, "neither CRENDER_ENV_REFLECT nor CRENDER_ENV_BACKGROUND");
    if (T == 0 || reflectivity == 0.0f) reflect = false;       // no covered pixel is written
    if (!reflect && !background) return CRENDER_OK;
    const ProjConst P = make_proj(P16, W, H);
    EnvCall C{};
    for (int i = 0; i < 9; ++i) C.M[i] = M9[i];
    C.tint[0] = tint3[0]; C.tint[1] = tint3[1]; C.tint[2] = tint3[2];
    C.reflectivity = reflectivity;
    C.f0 = f0;
    C.one_minus_f0 = (float)(1.0 - (double)f0);
    C.gain = background_gain;
    C.frac = level_frac;
    C.xs = P.xs;
    C.ys = P.ys;
    if (background) {
        C.kx = (float)(1.0 / ((double)P.xs * (double)P16[0]));
        C.ky = (float)(1.0 / ((double)P.ys * (double)P16[5]));
    }
    C.S0 = S0;
    C.S1 = S1;
    // [reflect + 2 background - 1][two levels]
    static constexpr decltype(&k_env_shade<true, false, false>) kernels[3][2] = {
        {k_env_shade<true, false, false>, k_env_shade<true, false, true>},
        {k_env_shade<false, true, false>, k_env_shade<false, true, true>},
        {k_env_shade<true, true, false>, k_env_shade<true, true, true>}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[(reflect ? 1 : 0) + (background ? 2 : 0) - 1][two], G.grid, dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_winner, d_tri, T, d_pos_of, P, d_normal, d_faces0, d_faces1, C,
                       d_color, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_env_shade");
    return CRENDER_OK;
}

}  // extern "C"
