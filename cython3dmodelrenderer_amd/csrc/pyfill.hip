// pyfill.hip — the numpy filler of crender/py on gfx950 (include/crender_py.h): the reference's
// per-triangle AdvancedPixelBufferFiller.compute_triangle_statistics, fed triangle by triangle by the
// py Renderer, for a whole ordered sequence of triangles at once.
//
// Launches: k_py_check (domain), k_py_seed (CLEAR; key plane seeded from the z plane), k_py_setup (one
// thread per triangle: culls, projection, box, float32 denominators; each workgroup scans its 256 box
// sizes), k_py_scan (one workgroup: the workgroups' totals into global offsets), then two walks over
// every box pixel of the draw, one pixel per work item of a fixed grid, so that a large triangle is
// spread over every CU: k_py_walk<kCount> counts each triangle's inside pixels (saturated at 2 in
// effect), k_py_walk<kKey> forms the depth keys with that count and takes their atomicMin; last
// k_py_resolve (one thread per pixel: the winner's z, normal and colour recomputed and stored).
// A work item finds its pixel's triangle by two binary searches: the workgroup offsets, then the
// triangle offsets inside that workgroup (empty boxes share the next offset; the last match holds it).
//
// Everything the reference computes in float64 is float64 here, every fma is written out and the
// library is built with -ffp-contract=off, so each value is the same expression with the same
// roundings as numpy's.
#include "common.h"
#include "../../include/crender_py.h"

using namespace crender_detail;

namespace {

constexpr int kMaxSide = 1 << 15;             // box sizes fit a uint32, keys' pixels an int32 index
constexpr int64_t kMaxT = (int64_t)1 << 30;   // ranks fit the key's 31-bit tiebreak
constexpr uint32_t kTieMax = 0x7fffffffu;
constexpr int kWalkBlocks = 2048;             // fixed grid of the walks (grid-stride over the pixels)

enum { kCount = 0, kKey = 1 };

// A triangle after setup: projected float32 vertices, the three float32 denominators, the box.
struct alignas(16) Rec {
    float x0, x1, x2, y0, y1, y2, z0, z1, z2, d0, d1, d2;
    int xl, yb, bw, bh;           // bw = bh = 0: culled or empty
};

CR_DEV bool finite(float v) { return fabsf(v) <= 3.402823466e38f; }

// float32 -> int32 as x86's cvttss2si: NaN or out of range -> INT_MIN (ceil is applied before)
CR_DEV int x86_i32(float v)
{
    return (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u;
}

// float64 -> uint8 as numpy's C cast on x86-64: cvttsd2si to int32 (NaN / out of range -> INT_MIN), low byte
CR_DEV uint8_t x86_u8(double v)
{
    return (v > -2147483649.0 && v < 2147483648.0) ? (uint8_t)(int)v : (uint8_t)0;
}

// np.min / np.max of three float32: a NaN wins
CR_DEV float nmin3(float a, float b, float c)
{
    if (a != a || b != b || c != c) return __builtin_nanf("");
    return fminf(fminf(a, b), c);
}
CR_DEV float nmax3(float a, float b, float c)
{
    if (a != a || b != b || c != c) return __builtin_nanf("");
    return fmaxf(fmaxf(a, b), c);
}

// advanced_pixel_buffer_filler.py:176-178 at pixel (x, y)
CR_DEV void bary(const Rec &r, int x, int y, double &l0, double &l1, double &l2)
{
    const double X = (double)x, Y = (double)y;
    const float a0 = r.x1 - r.x2, b0 = r.y1 - r.y2;
    const float a1 = r.x2 - r.x0, b1 = r.y2 - r.y0;
    const float a2 = r.x0 - r.x1, b2 = r.y0 - r.y1;
    l0 = ((double)a0 * (Y - (double)r.y2) - (double)b0 * (X - (double)r.x2)) / (double)r.d0;
    l1 = ((double)a1 * (Y - (double)r.y0) - (double)b1 * (X - (double)r.x0)) / (double)r.d1;
    l2 = ((double)a2 * (Y - (double)r.y1) - (double)b2 * (X - (double)r.x1)) / (double)r.d2;
}

// :224: the dgemv order for n >= 2 inside pixels, the ddot order for n = 1
CR_DEV double depth(const Rec &r, uint32_t n, double l0, double l1, double l2)
{
    if (n >= 2) return fma(l2, (double)r.z2, fma(l0, (double)r.z0, l1 * (double)r.z1));
    return fma(l2, (double)r.z2, fma(l1, (double)r.z1, l0 * (double)r.z0));
}

CR_DEV double interp(double l0, double l1, double l2, float v0, float v1, float v2)
{
    return fma(l2, (double)v2, fma(l1, (double)v1, l0 * (double)v0));
}

// order-preserving bits of a float32 (-0 taken as +0); NaN orders below everything (nothing beats it)
CR_DEV uint32_t ordered(float f)
{
    if (f != f) return 0u;
    uint32_t u = __float_as_uint(f);
    if (f == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

CR_DEV uint64_t make_key(uint32_t ob, uint32_t cls, uint32_t tie)
{
    return ((uint64_t)ob << 32) | ((uint64_t)cls << 31) | tie;
}

CR_DEV uint32_t key_rank(uint64_t k)
{
    const uint32_t tie = (uint32_t)k & kTieMax;
    return ((uint32_t)k >> 31) ? tie : kTieMax - tie;
}

// Domain check of every input value (any thread that finds one out sets *status).
__global__ __launch_bounds__(kThreads) void k_py_check(const float *__restrict__ tri, const float *__restrict__ col,
                                                        const float *__restrict__ nrm, int64_t n,
                                                        int32_t *__restrict__ status)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const float v = tri[i];
        bad |= !finite(v) || !finite(col[i]) || !finite(nrm[i]) || (i % 3 == 2 && v == 0.0f);
    }
    if (wave_any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

// CLEAR, then the key plane seeded with the pixel's current z as rank 0 (class 1, tiebreak 0).
__global__ __launch_bounds__(kThreads) void k_py_seed(float *__restrict__ z, uint8_t *__restrict__ cb,
                                                       float *__restrict__ nb, uint64_t *__restrict__ key,
                                                       size_t npix, int clear, const int32_t *__restrict__ status)
{
    if (*status) return;
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += stride) {
        if (clear) {
            z[i] = 1e6f;
            cb[i * 3] = cb[i * 3 + 1] = cb[i * 3 + 2] = 0;
            nb[i * 3] = nb[i * 3 + 1] = nb[i * 3 + 2] = 0.0f;
        }
        key[i] = make_key(ordered(z[i]), 1u, 0u);
    }
}

// Inclusive sum of v over the workgroup (uint64: 256 boxes of up to 2^30 pixels); s holds the sums
// afterwards, s[kThreads - 1] the total.  Every thread of the workgroup must call it.
CR_DEV uint64_t block_incl_scan(uint64_t v, uint64_t *s)
{
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const uint64_t add = tid >= d ? s[tid - d] : 0ull;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    return s[tid];
}

// :59-71 and :84-145 for one triangle
CR_DEV Rec setup_one(const float *v, const float *n, float p00, float p11, float p22, float p32, int H, int W)
{
    Rec r;
    // :59 degenerate in raw x / y
    const float ax = v[3] - v[0], ay = v[4] - v[1], bx = v[6] - v[0], by = v[7] - v[1];
    const float cross = ax * by - ay * bx;
    // :66 back-facing: the float64 dot of [0, 0, 1] with the float32 mean normal is >= 0
    const float sx = (n[0] + n[3]) + n[6], sy = (n[1] + n[4]) + n[7], sz = (n[2] + n[5]) + n[8];
    // (the mean's sign: sz / 3 rounds a sum of -2^-149 to -0, which is culled)
    const bool culled = cross == 0.0f || (finite(sx) && finite(sy) && sz / 3.0f >= 0.0f);
    // :84-105 projection, float32
    const float hw = (float)W * 0.5f, hh = (float)H * 0.5f;
    float px[3], py[3], pz[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = v[k * 3], y = v[k * 3 + 1], z = v[k * 3 + 2];
        const float cz = z * p22 + p32;
        px[k] = (x * p00 / z + 1.0f) * hw;
        py[k] = (y * p11 / z + 1.0f) * hh;
        pz[k] = cz / z;
    }
    r.x0 = px[0]; r.x1 = px[1]; r.x2 = px[2];
    r.y0 = py[0]; r.y1 = py[1]; r.y2 = py[2];
    r.z0 = pz[0]; r.z1 = pz[1]; r.z2 = pz[2];
    r.d0 = (r.x1 - r.x2) * (r.y0 - r.y2) - (r.y1 - r.y2) * (r.x0 - r.x2);
    r.d1 = (r.x2 - r.x0) * (r.y1 - r.y0) - (r.y2 - r.y0) * (r.x1 - r.x0);
    r.d2 = (r.x0 - r.x1) * (r.y2 - r.y1) - (r.y0 - r.y1) * (r.x2 - r.x1);
    // :130-145 box
    int xl = x86_i32(ceilf(nmin3(px[0], px[1], px[2]))), xr = x86_i32(ceilf(nmax3(px[0], px[1], px[2])));
    int yb = x86_i32(ceilf(nmin3(py[0], py[1], py[2]))), yt = x86_i32(ceilf(nmax3(py[0], py[1], py[2])));
    xl = min(max(xl, 0), W); xr = min(max(xr, 0), W);
    yb = min(max(yb, 0), H); yt = min(max(yt, 0), H);
    r.xl = xl;
    r.yb = yb;
    r.bw = (culled || xr <= xl || yt <= yb) ? 0 : xr - xl;
    r.bh = r.bw ? yt - yb : 0;
    return r;
}

// One thread per triangle: :59-71 and :84-145.
__global__ __launch_bounds__(kThreads) void k_py_setup(const float *__restrict__ tri, const float *__restrict__ nrm,
                                                        int64_t T, float p00, float p11, float p22, float p32,
                                                        int H, int W, Rec *__restrict__ rec,
                                                        uint64_t *__restrict__ toff, uint32_t *__restrict__ cnt,
                                                        uint64_t *__restrict__ boff,
                                                        const int32_t *__restrict__ status)
{
    if (*status) return;
    __shared__ uint64_t s_sum[kThreads];
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * kThreads + tid;
    uint64_t size = 0;
    if (t < T) {
        const Rec r = setup_one(tri + t * 9, nrm + t * 9, p00, p11, p22, p32, H, W);
        rec[t] = r;
        cnt[t] = 0u;
        size = (uint64_t)(uint32_t)r.bw * (uint32_t)r.bh;
    }
    const uint64_t incl = block_incl_scan(size, s_sum);
    if (t < T) toff[t] = incl - size;
    if (tid == kThreads - 1) boff[blockIdx.x] = incl;
}

// One workgroup: boff[0 .. nb) (the workgroups' box totals) becomes their exclusive offsets, in place,
// and boff[nb] the draw's total.
__global__ __launch_bounds__(kThreads) void k_py_scan(uint64_t *__restrict__ boff, int64_t nb,
                                                       const int32_t *__restrict__ status)
{
    if (*status) return;
    __shared__ uint64_t s_sum[kThreads];
    uint64_t carry = 0;
    for (int64_t base = 0; base < nb; base += kThreads) {
        const int64_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? boff[i] : 0ull;
        const uint64_t incl = block_incl_scan(v, s_sum);
        if (i < nb) boff[i] = carry + incl - v;
        carry += s_sum[kThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) boff[nb] = carry;
}

// Every box pixel of the draw, one per work item of a fixed grid.  PASS kCount: each inside pixel adds
// to its triangle's count while the count is below 2 (it ends at min(n, 2) or a little above: only
// n >= 2 against n = 1 is read).  PASS kKey: the depth keys, with that count.
template <int PASS>
__global__ __launch_bounds__(kThreads) void k_py_walk(const Rec *__restrict__ rec, const uint64_t *__restrict__ toff,
                                                       const uint64_t *__restrict__ boff, int64_t T, int W,
                                                       uint32_t *__restrict__ cnt, uint64_t *__restrict__ key,
                                                       const int32_t *__restrict__ status)
{
    if (*status) return;
    const int64_t nb = (T + kThreads - 1) / kThreads;
    const uint64_t total = boff[nb];
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < total; p += stride) {
        // the last workgroup, then the last triangle in it, whose first pixel is at or before p
        int64_t lo = 0, hi = nb - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (boff[mid] <= p) lo = mid; else hi = mid - 1;
        }
        const uint64_t in_block = p - boff[lo];
        const int64_t first = lo * kThreads;
        int jl = 0, jh = (int)min((int64_t)kThreads, T - first) - 1;
        while (jl < jh) {
            const int mid = (jl + jh + 1) >> 1;
            if (toff[first + mid] <= in_block) jl = mid; else jh = mid - 1;
        }
        const int64_t t = first + jl;
        const Rec r = rec[t];
        const uint32_t q = (uint32_t)(in_block - toff[t]);
        const int x = r.xl + (int)(q % (uint32_t)r.bw), y = r.yb + (int)(q / (uint32_t)r.bw);
        double l0, l1, l2;
        bary(r, x, y, l0, l1, l2);
        if (!(l0 >= 0.0 && l1 >= 0.0 && l2 >= 0.0)) continue;
        if (PASS == kCount) {
            if (__hip_atomic_load(cnt + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 2u)
                atomicAdd(cnt + t, 1u);
            continue;
        }
        const double z = depth(r, cnt[t], l0, l1, l2);
        if (!(z >= 0.0 && z <= 1.0)) continue;
        const float zf = (float)z;
        const uint32_t rank = (uint32_t)t + 1u;
        const uint64_t k = (z < (double)zf) ? make_key(ordered(zf), 0u, kTieMax - rank)
                                            : make_key(ordered(zf), 1u, rank);
        atomicMin((unsigned long long *)(key + (size_t)y * W + x), (unsigned long long)k);
    }
}

// One thread per pixel: the key's winner, if a triangle, stores its z, normal and colour.
__global__ __launch_bounds__(kThreads) void k_py_resolve(const Rec *__restrict__ rec, const uint32_t *__restrict__ cnt,
                                                          const float *__restrict__ col, const float *__restrict__ nrm,
                                                          const uint64_t *__restrict__ key, float *__restrict__ z,
                                                          uint8_t *__restrict__ cb, float *__restrict__ nb, int H,
                                                          int W, const int32_t *__restrict__ status)
{
    if (*status) return;
    const size_t npix = (size_t)H * W;
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t pix = (size_t)blockIdx.x * kThreads + threadIdx.x; pix < npix; pix += stride) {
        const uint32_t rank = key_rank(key[pix]);
        if (rank == 0u) continue;
        const int64_t t = (int64_t)rank - 1;
        const Rec r = rec[t];
        const int y = (int)(pix / (size_t)W), x = (int)(pix - (size_t)y * W);
        double l0, l1, l2;
        bary(r, x, y, l0, l1, l2);
        z[pix] = (float)depth(r, cnt[t], l0, l1, l2);
        const float *n = nrm + t * 9, *c = col + t * 9;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            nb[pix * 3 + k] = (float)interp(l0, l1, l2, n[k], n[3 + k], n[6 + k]);
            cb[pix * 3 + k] = x86_u8(interp(l0, l1, l2, c[k], c[3 + k], c[6 + k]));
        }
    }
}

// guro_illumination.py:20-27 on the uint8 colour plane
__global__ __launch_bounds__(kThreads) void k_py_guro(uint8_t *__restrict__ cb, const float *__restrict__ nb,
                                                       float l0, float l1, float l2, size_t npix)
{
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += stride) {
        const float n0 = nb[i * 3], n1 = nb[i * 3 + 1], n2 = nb[i * 3 + 2];
        const float s = ((0.0f + n0 * l0) + n1 * l1) + n2 * l2;
        const float m = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
        float c = s / (m + 1e-6f);
        c = c < 0.0f ? 0.0f : c;  // np.clip keeps a NaN a NaN
        c = c > 1.0f ? 1.0f : c;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = (float)cb[i * 3 + k] * c;          // in [0, 255] or NaN
            cb[i * 3 + k] = v == v ? (uint8_t)(int)v : (uint8_t)0;
        }
    }
}

// Scratch: the key plane, then per triangle its Rec, box offset and inside count, then the
// workgroups' offsets and the total; each part 16-byte aligned.
struct Layout {
    size_t rec, toff, cnt, boff, bytes;
};

Layout layout(int H, int W, int64_t T)
{
    const auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t nb = (size_t)((T + kThreads - 1) / kThreads);
    Layout L;
    L.rec = up((size_t)H * W * sizeof(uint64_t));
    L.toff = L.rec + up((size_t)T * sizeof(Rec));
    L.cnt = L.toff + up((size_t)T * sizeof(uint64_t));
    L.boff = L.cnt + up((size_t)T * sizeof(uint32_t));
    L.bytes = L.boff + up((nb + 1) * sizeof(uint64_t));
    return L;
}

}  // namespace

extern "C" {

size_t crender_py_scratch_bytes(int H, int W, int64_t T)
{
    if (H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide || T < 0 || T >= kMaxT) return 0;
    return layout(H, W, T).bytes;
}

int crender_py_draw(const float *d_tri, const float *d_col, const float *d_nrm, int64_t T, const float *proj4,
                    float *d_z, uint8_t *d_color, float *d_normal, int H, int W, unsigned flags, void *d_scratch,
                    int32_t *d_status, void *stream)
{
    if (T < 0 || T >= kMaxT || H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide || !proj4 || !d_z || !d_color ||
        !d_normal || !d_scratch || !d_status || (flags & ~(unsigned)CRENDER_PY_CLEAR) ||
        (T > 0 && (!d_tri || !d_col || !d_nrm)) || ((uintptr_t)d_scratch & 15))
        return fail(CRENDER_EINVAL, "crender_py_draw: bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t npix = (size_t)H * W;
    const Layout L = layout(H, W, T);
    char *base = static_cast<char *>(d_scratch);
    uint64_t *key = reinterpret_cast<uint64_t *>(base);
    Rec *rec = reinterpret_cast<Rec *>(base + L.rec);
    uint64_t *toff = reinterpret_cast<uint64_t *>(base + L.toff);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(base + L.cnt);
    uint64_t *boff = reinterpret_cast<uint64_t *>(base + L.boff);
    CR_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
    if (T > 0) {
        hipLaunchKernelGGL(k_py_check, dim3(grid_for((size_t)T * 9, 2048)), dim3(kThreads), 0, st, d_tri, d_col,
                           d_nrm, T * 9, d_status);
        CR_LAUNCH_CHECK("k_py_check");
    }
    hipLaunchKernelGGL(k_py_seed, dim3(grid_for(npix, 4096)), dim3(kThreads), 0, st, d_z, d_color, d_normal, key,
                       npix, (flags & CRENDER_PY_CLEAR) ? 1 : 0, d_status);
    CR_LAUNCH_CHECK("k_py_seed");
    if (T == 0) return CRENDER_OK;
    const int64_t nb = (T + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_py_setup, dim3((unsigned)nb), dim3(kThreads), 0, st, d_tri, d_nrm, T, proj4[0], proj4[1],
                       proj4[2], proj4[3], H, W, rec, toff, cnt, boff, d_status);
    CR_LAUNCH_CHECK("k_py_setup");
    hipLaunchKernelGGL(k_py_scan, dim3(1), dim3(kThreads), 0, st, boff, nb, d_status);
    CR_LAUNCH_CHECK("k_py_scan");
    hipLaunchKernelGGL(k_py_walk<kCount>, dim3(kWalkBlocks), dim3(kThreads), 0, st, rec, toff, boff, T, W, cnt, key,
                       d_status);
    CR_LAUNCH_CHECK("k_py_walk<count>");
    hipLaunchKernelGGL(k_py_walk<kKey>, dim3(kWalkBlocks), dim3(kThreads), 0, st, rec, toff, boff, T, W, cnt, key,
                       d_status);
    CR_LAUNCH_CHECK("k_py_walk<key>");
    hipLaunchKernelGGL(k_py_resolve, dim3(grid_for(npix, 4096)), dim3(kThreads), 0, st, rec, cnt, d_col, d_nrm,
                       key, d_z, d_color, d_normal, H, W, d_status);
    CR_LAUNCH_CHECK("k_py_resolve");
    return CRENDER_OK;
}

int crender_py_guro(uint8_t *d_color, const float *d_normal, const float *light3, int H, int W, void *stream)
{
    if (!d_color || !d_normal || !light3 || H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide)
        return fail(CRENDER_EINVAL, "crender_py_guro: bad argument");
    const size_t npix = (size_t)H * W;
    hipLaunchKernelGGL(k_py_guro, dim3(grid_for(npix, 4096)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       d_color, d_normal, light3[0], light3[1], light3[2], npix);
    CR_LAUNCH_CHECK("k_py_guro");
    return CRENDER_OK;
}

}  // extern "C"
