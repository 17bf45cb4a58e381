// resolve.hip — the supersampling resolve (include/crender_ssaa.h states the arithmetic; this file keeps its
// operation order): s x s source pixels averaged into one output pixel, with the illumination and the uint8
// presentation fused in, so that the supersampled planes are read once and never rewritten.
//
// A pixel of the OUTPUT per work item, 64 consecutive output pixels of one output row per wavefront: its lanes
// read 64 * 12 * s contiguous bytes of each of the s source rows.  A lane's 12 * s bytes of a row are taken VEC
// floats at a time, VEC the widest of 4, 2, 1 that divides s: three loads of VEC floats are VEC whole samples, and
// 12 * s * k bytes into a plane is a multiple of 16 for s = 4 and 8, of 8 for even s — the loads are as aligned as
// the plane itself (the vector types below promise the compiler no more than a float's alignment, so a plane at
// an odd address is read correctly too).  S = 1 .. 4 are unrolled; S = 0 is the loop for 5 .. 8, in the same
// visiting order.
//
// The sum is one accumulator per channel and lane, in the contract's row-major order: float32 addition does
// not associate, so nothing is reduced across lanes.
//
// uint8 output: a lane's three bytes are packed into a register and a wavefront's 192 bytes leave as 48 dword
// stores — dword d holds bytes 4d .. 4d + 3 of the run, the tail of pixel q = 4d / 3 and the head of pixel
// q + 1, fetched with two cross-lane reads.  (A byte store per channel would be 192 store instructions' worth
// of the slowest store of the chip.)  A row of Wo * 3 bytes starts wherever the one before it ended, so these
// stores are not aligned to their size: global memory takes them as they are.  Only the last wavefront of a
// row, when Wo * 3 is no multiple of 4, ends with up to three byte stores.
#include "common.h"
#include "../../include/crender_ssaa.h"

using namespace crender_detail;

namespace {

typedef uint32_t u32_any __attribute__((aligned(1)));     // a dword at any byte address
typedef float f32x2 __attribute__((ext_vector_type(2), aligned(4)));
typedef float f32x4 __attribute__((ext_vector_type(4), aligned(4)));

// 3 * VEC consecutive floats = VEC samples, as three loads of VEC floats
template <int VEC>
CR_DEV void load_group(const float *__restrict__ p, float v[3 * VEC])
{
    if constexpr (VEC == 4) {
        const f32x4 *q = reinterpret_cast<const f32x4 *>(p);
        const f32x4 a = q[0], b = q[1], c = q[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else if constexpr (VEC == 2) {
        const f32x2 *q = reinterpret_cast<const f32x2 *>(p);
        const f32x2 a = q[0], b = q[1], c = q[2];
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    }
}

// VEC samples of one source row added to the accumulators, left to right; `first`: the group starts with
// sample (0, 0), which the sum starts FROM.
template <int VEC, bool LIGHT>
CR_DEV void add_group(const float *__restrict__ cp, const float *__restrict__ np_, const Light &L, bool first,
                      float acc[3])
{
    float c[3 * VEC], n[3 * VEC];
    load_group<VEC>(cp, c);
    if constexpr (LIGHT) load_group<VEC>(np_, n);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        float c0 = c[3 * k], c1 = c[3 * k + 1], c2 = c[3 * k + 2];
        if constexpr (LIGHT) {
            const float f = guro_factor(L, n[3 * k], n[3 * k + 1], n[3 * k + 2]);
            c0 = c0 * f; c1 = c1 * f; c2 = c2 * f;
        }
        const bool start = first && k == 0;
        acc[0] = start ? c0 : acc[0] + c0;
        acc[1] = start ? c1 : acc[1] + c1;
        acc[2] = start ? c2 : acc[2] + c2;
    }
}

// crender_present_u8's cast (model_ops.hip): cvttss2si, then the low byte
CR_DEV uint32_t u8_of(float v)
{
    int iv = (int)0x80000000;
    if (v > -2147483904.0f && v < 2147483648.0f) iv = (int)v;
    return (uint32_t)iv & 0xFFu;
}

template <int S, int VEC, bool LIGHT, bool U8>
__global__ __launch_bounds__(kThreads) void k_ssaa(const float *__restrict__ cb, const float *__restrict__ nb, Light L,
                                                   int W, int Wo, int Ho, int s_any, int Y0, int Y1,
                                                   void *__restrict__ out, int flip)
{
    const int s = S ? S : s_any;
    const int lane = threadIdx.x & 63;
    const int X = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    const bool inside = X < Wo;
    const float fs2 = (float)(s * s);
    const size_t row_floats = (size_t)W * 3, out_row = (size_t)Wo * 3;
    const size_t at = (size_t)X * (size_t)(3 * s);
    for (int Y = Y0 + (int)blockIdx.y; Y < Y1; Y += (int)gridDim.y) {
        float r[3] = {0.0f, 0.0f, 0.0f};
        if (inside) {
            const size_t first_row = (size_t)Y * (size_t)s;
            if constexpr (S != 0) {
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    const size_t o = (first_row + j) * row_floats + at;
#pragma unroll
                    for (int g = 0; g < S / VEC; ++g)
                        add_group<VEC, LIGHT>(cb + o + g * 3 * VEC, LIGHT ? nb + o + g * 3 * VEC : nullptr, L,
                                              j == 0 && g == 0, r);
                }
            } else {
                const int groups = s / VEC;
                for (int j = 0; j < s; ++j) {
                    const size_t o = (first_row + j) * row_floats + at;
                    for (int g = 0; g < groups; ++g)
                        add_group<VEC, LIGHT>(cb + o + g * 3 * VEC, LIGHT ? nb + o + g * 3 * VEC : nullptr, L,
                                              j == 0 && g == 0, r);
                }
            }
            r[0] = r[0] / fs2; r[1] = r[1] / fs2; r[2] = r[2] / fs2;
        }
        const size_t Yo = (size_t)(flip ? Ho - 1 - Y : Y);
        if constexpr (!U8) {
            if (inside) {
                float *op = reinterpret_cast<float *>(out) + Yo * out_row + (size_t)X * 3;
                op[0] = r[0]; op[1] = r[1]; op[2] = r[2];
            }
        } else {
            // every lane of the wavefront takes part in the cross-lane reads, inside the row or not
            const uint32_t p = inside ? (u8_of(r[0]) | u8_of(r[1]) << 8 | u8_of(r[2]) << 16) : 0u;
            const int q = (4 * lane) / 3;                     // the pixel (lane) byte 4 * lane of the run belongs to
            const uint32_t lo = (uint32_t)__shfl((int)p, q & 63, 64);
            const uint32_t hi = (uint32_t)__shfl((int)p, (q + 1) & 63, 64);
            const unsigned long long two = (unsigned long long)lo | ((unsigned long long)hi << 24);
            const uint32_t word = (uint32_t)(two >> (8 * (4 * lane - 3 * q)));
            const int wave_x = X - lane;                      // first pixel of the wavefront's run
            int n = Wo - wave_x;                              // pixels of the run inside the row
            n = n < 0 ? 0 : (n > 64 ? 64 : n);
            const int nbytes = 3 * n, whole = nbytes >> 2;
            unsigned char *op = reinterpret_cast<unsigned char *>(out) + Yo * out_row + (size_t)wave_x * 3 +
                                (size_t)lane * 4;
            if (lane < whole) {
                *reinterpret_cast<u32_any *>(op) = word;
            } else if (lane == whole) {
                const int rest = nbytes & 3;                  // the row's tail
                if (rest > 0) op[0] = (unsigned char)(word & 0xFFu);
                if (rest > 1) op[1] = (unsigned char)((word >> 8) & 0xFFu);
                if (rest > 2) op[2] = (unsigned char)((word >> 16) & 0xFFu);
            }
        }
    }
}

struct Call {
    const float *cb, *nb;
    Light L;
    int W, Wo, Ho, s, Y0, Y1;
    void *out;
    int flip;
    dim3 grid;
    hipStream_t st;
};

template <int S, int VEC>
void launch(const Call &c, bool light, bool u8)
{
#define CR_SSAA_LAUNCH(LIGHT, U8)                                                                              \
    hipLaunchKernelGGL((k_ssaa<S, VEC, LIGHT, U8>), c.grid, dim3(kThreads), 0, c.st, c.cb, c.nb, c.L, c.W, c.Wo, \
                       c.Ho, c.s, c.Y0, c.Y1, c.out, c.flip)
    if (light) {
        if (u8) CR_SSAA_LAUNCH(true, true); else CR_SSAA_LAUNCH(true, false);
    } else {
        if (u8) CR_SSAA_LAUNCH(false, true); else CR_SSAA_LAUNCH(false, false);
    }
#undef CR_SSAA_LAUNCH
}

}  // namespace

extern "C" {

int crender_ssaa_resolve(const float *d_color, const float *d_normal, const float *light3, int H, int W, int s,
                         int Y0, int Y1, void *d_out, unsigned flags, void *stream)
{
    if (!d_color || !d_out) return fail(CRENDER_EINVAL, "crender_ssaa_resolve: d_color or d_out is NULL");
    if (s < 1 || s > CRENDER_SSAA_MAX) return fail(CRENDER_EINVAL, "crender_ssaa_resolve: s outside 1 .. 8");
    if (H < 1 || W < 1 || H % s || W % s)
        return fail(CRENDER_EINVAL, "crender_ssaa_resolve: H or W is below 1 or no multiple of s");
    const int Ho = H / s, Wo = W / s;
    if (Y0 < 0 || Y1 > Ho || Y0 >= Y1) return fail(CRENDER_EINVAL, "crender_ssaa_resolve: rows outside the output");
    if (light3 && !d_normal) return fail(CRENDER_EINVAL, "crender_ssaa_resolve: a light without normals");
    if (d_normal && !light3) return fail(CRENDER_EINVAL, "crender_ssaa_resolve: normals without a light");
    if (flags & ~(unsigned)(CRENDER_SSAA_U8 | CRENDER_SSAA_FLIP))
        return fail(CRENDER_EINVAL, "crender_ssaa_resolve: unknown flag bits");
    const bool light = light3 != nullptr, u8 = (flags & CRENDER_SSAA_U8) != 0;
    const int rows = Y1 - Y0;
    Call c{d_color, d_normal, light ? Light{light3[0], light3[1], light3[2], 1} : Light{0.0f, 0.0f, 0.0f, 0},
           W, Wo, Ho, s, Y0, Y1, d_out, (flags & CRENDER_SSAA_FLIP) ? 1 : 0,
           dim3((unsigned)((Wo + kThreads - 1) / kThreads), (unsigned)(rows < 65535 ? rows : 65535)),
           static_cast<hipStream_t>(stream)};
    switch (s) {
    case 1: launch<1, 1>(c, light, u8); break;
    case 2: launch<2, 2>(c, light, u8); break;
    case 3: launch<3, 1>(c, light, u8); break;
    case 4: launch<4, 4>(c, light, u8); break;
    case 6: launch<0, 2>(c, light, u8); break;
    case 8: launch<0, 4>(c, light, u8); break;
    default: launch<0, 1>(c, light, u8); break;      // 5, 7
    }
    CR_LAUNCH_CHECK("k_ssaa");
    return CRENDER_OK;
}

}  // extern "C"
