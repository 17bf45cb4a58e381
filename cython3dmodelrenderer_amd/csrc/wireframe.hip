// wireframe.hip — EdgeOnlyPixelBufferFiller on gfx950 (include/crender_wire.h): the reference's
// per-pixel Bresenham loop (line_bresenham.py:6-45) for a whole mesh at once.
//
// Every line ("segment": an edge, or a vertex in dots mode, which is a line of length 0) is
// clipped to the frame by its own thread — the window of t along the major axis, narrowed by
// inverting k(t) for the minor one, so that every candidate it counts lands on screen — and a
// workgroup then walks the candidate pixels of its 256 segments, one per work item, finding each
// one's segment by a binary search over the workgroup's scan of the counts in LDS.  No device-wide
// scan and no host round trip: a launch sizes nothing from another launch's result.
//
// Also here: the hidden-line overlay over the winner plane of AdvancedPixelBufferFiller (k_wire_overlay, at the end
// of the file), a deferred pass of the shape of k_phong_shade.
//
// Order.  With one constant colour every writer of a pixel stores the same 12 bytes.  With
// per-triangle colours the last write of the reference's sequence (triangle i, edge e) wins; a line
// never visits a pixel twice (its major coordinate moves at every step), so the winner is the
// segment with the largest 3 i + e: one launch takes the atomic maximum of 3 i + e + 1 per pixel in
// a uint32 key plane, a second one walks the same pixels again and the segment that finds its own
// key stores its colour and writes the key back to 0.
#include <math.h>

#include "common.h"
#include "../../include/crender_wire.h"

using namespace crender_detail;

#include "winner_pass.h"     // WinnerPixel, gather_corners, pass_grid (k_wire_overlay)

namespace {

constexpr float kDomain = 1073741824.0f;     // 2^30: |c| below it keeps 2 t es within int64
constexpr int kMaxSide = 1 << 20;            // 256 segments x 2^20 candidates fit a uint32 count

enum { kStoreConst = 0, kKeyMax = 1, kResolve = 2 };

CR_DEV int64_t floor_div(int64_t n, int64_t d)       // d > 0
{
    int64_t q = n / d;
    if (n - q * d != 0 && n < 0) --q;
    return q;
}

// A segment from (x1, y1) to (x2, y2) in the reference's terms: major axis a (x if |dx| > |dy|, else
// y: ties go to y), minor axis b, lengths el >= es, steps sa, sb; t0 = first t on screen.
struct Seg {
    int a1, b1, el, es, t0, sg;      // sg: x-major | (sa + 1) << 1 | (sb + 1) << 3
};

CR_DEV uint32_t seg_setup(int x1, int y1, int x2, int y2, int W, int H, Seg &s)
{
    const int dx = x2 - x1, dy = y2 - y1;                 // |x| < 2^30: no overflow
    const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0);
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    const bool xm = ax > ay;
    const int a1 = xm ? x1 : y1, b1 = xm ? y1 : x1;
    const int sa = xm ? sx : sy, sb = xm ? sy : sx;
    const int Ma = xm ? W : H, Mb = xm ? H : W;
    const int el = xm ? ax : ay, es = xm ? ay : ax;
    // major axis: a1 + sa t in [0, Ma), t in [0, el]
    int64_t lo = 0, hi = el;
    if (sa > 0) {
        lo = max(lo, (int64_t)-a1);
        hi = min(hi, (int64_t)Ma - 1 - a1);
    } else if (sa < 0) {
        lo = max(lo, (int64_t)a1 - (Ma - 1));
        hi = min(hi, (int64_t)a1);
    } else if (a1 < 0 || a1 >= Ma) {
        hi = -1;
    }
    // minor axis: b1 + sb k in [0, Mb), k = k(t) in [0, es], non-decreasing in t
    int64_t klo = 0, khi = es;
    if (sb > 0) {
        klo = max(klo, (int64_t)-b1);
        khi = min(khi, (int64_t)Mb - 1 - b1);
    } else if (sb < 0) {
        klo = max(klo, (int64_t)b1 - (Mb - 1));
        khi = min(khi, (int64_t)b1);
    } else if (b1 < 0 || b1 >= Mb) {
        khi = -1;
    }
    if (klo > khi) {
        hi = -1;
    } else if (es > 0) {
        // k(t) >= K  <=>  t >= floor((2 el K - el) / (2 es)) + 1;  k(t) <= K  <=>  t <= floor((2 el K + el) / (2 es))
        const int64_t EL = el, ES = es;
        lo = max(lo, floor_div(2 * EL * klo - EL, 2 * ES) + 1);
        hi = min(hi, floor_div(2 * EL * khi + EL, 2 * ES));
    }
    s.a1 = a1; s.b1 = b1; s.el = el; s.es = es;
    s.t0 = (int)max(lo, (int64_t)0);
    s.sg = (xm ? 1 : 0) | ((sa + 1) << 1) | ((sb + 1) << 3);
    return hi >= lo ? (uint32_t)(hi - lo + 1) : 0u;
}

// Pixel t of the segment: (major, minor) = (a1 + sa t, b1 + sb k(t)), k(t) = ceil((2 t es - el) / (2 el)).
CR_DEV void seg_pixel(const Seg &s, int64_t t, int &x, int &y)
{
    const int64_t k = s.el ? -floor_div((int64_t)s.el - 2 * t * s.es, 2 * (int64_t)s.el) : 0;
    const int sa = ((s.sg >> 1) & 3) - 1, sb = ((s.sg >> 3) & 3) - 1;
    const int a = s.a1 + sa * (int)t, b = s.b1 + sb * (int)k;
    x = (s.sg & 1) ? a : b;
    y = (s.sg & 1) ? b : a;
}

// Any x / y coordinate out of the domain (NaN, +-inf, |c| >= 2^30): *status = 1.
__global__ __launch_bounds__(kThreads) void k_wire_check(const float *__restrict__ tri, int64_t nvert,
                                                          int32_t *__restrict__ status)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    bool bad = false;
    for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvert; v += stride) {
        const float x = tri[v * 3], y = tri[v * 3 + 1];
        bad |= !(fabsf(x) < kDomain) || !(fabsf(y) < kDomain);
    }
    if (wave_any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

// CRENDER_WIRE_CLEAR: the fillers' initial state, unless the domain check failed.
__global__ __launch_bounds__(kThreads) void k_wire_clear(float *__restrict__ z, float *__restrict__ cb,
                                                          float *__restrict__ nb, size_t npix,
                                                          const int32_t *__restrict__ status)
{
    if (*status) return;
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += stride) {
        z[i] = 1e6f;
        cb[i * 3] = cb[i * 3 + 1] = cb[i * 3 + 2] = 0.0f;
        nb[i * 3] = nb[i * 3 + 1] = nb[i * 3 + 2] = 0.0f;
    }
}

// One workgroup per 256 segments (segment s = 3 i + e); MODE: kStoreConst / kKeyMax / kResolve.
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_wire(const float *__restrict__ tri, const float *__restrict__ col,
                                                    int64_t nseg, int dots, float c0, float c1, float c2,
                                                    float *__restrict__ cb, uint32_t *__restrict__ key,
                                                    int H, int W, const int32_t *__restrict__ status)
{
    if (*status) return;
    __shared__ int s_a1[kThreads], s_b1[kThreads], s_el[kThreads], s_es[kThreads], s_t0[kThreads],
        s_sg[kThreads];
    __shared__ uint32_t s_off[kThreads];
    __shared__ uint32_t s_wave[kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * kThreads;
    const int64_t seg = first + tid;
    uint32_t cnt = 0;
    Seg s = {0, 0, 0, 0, 0, 0};
    if (seg < nseg) {
        const int64_t i = seg / 3;
        const int e = (int)(seg - 3 * i);
        const int va = e, vb = dots ? e : (e == 2 ? 0 : e + 1);
        const float *v = tri + i * 9;
        // int() of the reference: truncation toward zero (in the domain: k_wire_check)
        cnt = seg_setup((int)v[va * 3], (int)v[va * 3 + 1], (int)v[vb * 3], (int)v[vb * 3 + 1], W, H, s);
    }
    s_a1[tid] = s.a1; s_b1[tid] = s.b1; s_el[tid] = s.el; s_es[tid] = s.es; s_t0[tid] = s.t0; s_sg[tid] = s.sg;
    // exclusive scan of the counts over the workgroup
    const uint32_t incl = wave_incl_sum(cnt);
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        base += w < (tid >> 6) ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    s_off[tid] = base + incl - cnt;
    __syncthreads();
    for (uint32_t p = tid; p < total; p += kThreads) {
        // the last segment whose first candidate is at or before p holds p (empty ones share the next offset)
        int j = 0;
#pragma unroll
        for (int step = kThreads / 2; step; step >>= 1)
            if (s_off[j + step] <= p) j += step;
        const Seg g = {s_a1[j], s_b1[j], s_el[j], s_es[j], s_t0[j], s_sg[j]};
        int x, y;
        seg_pixel(g, (int64_t)g.t0 + (p - s_off[j]), x, y);
        if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) continue;   // (clipped above; kept as a guard)
        const size_t pix = (size_t)y * W + x;
        const uint32_t me = (uint32_t)(first + j) + 1u;
        if (MODE == kStoreConst) {
            cb[pix * 3] = c0;
            cb[pix * 3 + 1] = c1;
            cb[pix * 3 + 2] = c2;
        } else if (MODE == kKeyMax) {
            atomicMax(key + pix, me);
        } else if (key[pix] == me) {
            const float *c = col + (size_t)(me - 1u) * 3;      // colors[i][e]: [T][3][3] = 3 floats per segment
            cb[pix * 3] = c[0];
            cb[pix * 3 + 1] = c[1];
            cb[pix * 3 + 2] = c[2];
            key[pix] = 0u;
        }
    }
}


// ---- the hidden-line overlay (crender_wire_overlay) -------------------------------------------------------------
// The shape of k_phong_shade (phong.hip): a pixel per work item, an 8 x 8 block of pixels per wavefront, a grid-stride
// loop over row blocks; a wavefront whose 64 winners are all background leaves after its one load.  A pixel sees the
// edges of its own winner only, so a line behind a nearer triangle is never drawn: no depth bias, no second look at z.

// The line and the window of a call.
struct WireStyle {
    float line[3], fill[3];
    float hi, feather, opacity;              // hi = width / 2 + feather / 2
};

// The statements "Per edge" of crender_wire.h: the distance of (fx, fy) to the line through a and b.
CR_DEV float line_distance(const float a[3], const float b[3], float fx, float fy)
{
    const float l1 = a[0] - b[0], l2 = a[1] - b[1];
    const float n = l1 * (fy - b[1]) - l2 * (fx - b[0]);
    const float len = sqrtf(l1 * l1 + l2 * l2);
    return fabsf(n) / len;
}

// FILL: every covered pixel is stored, over the fill colour; without it only the pixels on a line, over their own.
template <bool FILL>
__global__ __launch_bounds__(kThreads) void k_wire_overlay(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                            int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                            const uint8_t *__restrict__ edges, WireStyle S,
                                                            float *__restrict__ cb, int W, int y0, int y1, int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!wave_any(px.covered)) continue;        // a scalar branch: the whole wavefront leaves
        if (!px.covered) continue;
        unsigned mask = 7u;
        if (edges) mask = edges[px.orig];           // a scalar branch; the caller's order, as uv
        float c[3][3];
        gather_corners(tri, px.t, c[0], c[1], c[2]);
        project_vertex(P, c[0]);
        project_vertex(P, c[1]);
        project_vertex(P, c[2]);
        const float fx = (float)px.x, fy = (float)px.y;
        float m = INFINITY;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if (!((mask >> e) & 1u)) continue;
            const float d = line_distance(c[e], c[(e + 1) % 3], fx, fy);
            if (d < m) m = d;                       // (a NaN is never taken)
        }
        float a = (S.hi - m) / S.feather;
        const bool on = a > 0.0f;
        a = a > 1.0f ? 1.0f : a;
        a = a * S.opacity;
        float *cp = cb + px.pix * 3;
        if (FILL) {
            const float k = 1.0f - a;
#pragma unroll
            for (int j = 0; j < 3; ++j) cp[j] = on ? S.fill[j] * k + S.line[j] * a : S.fill[j];
        } else if (on) {
            const float k = 1.0f - a;
#pragma unroll
            for (int j = 0; j < 3; ++j) cp[j] = cp[j] * k + S.line[j] * a;
        }
    }
}

}  // namespace

extern "C" {

size_t crender_wire_key_bytes(int H, int W)
{
    if (H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide) return 0;
    return (size_t)H * W * sizeof(uint32_t);
}

int crender_wire_draw(const float *d_tri, const float *d_col, int64_t T, const float *line_bgr3, float *d_z,
                      float *d_color, float *d_normal, uint32_t *d_key, int H, int W, unsigned flags,
                      int32_t *d_status, void *stream)
{
    const bool force = flags & CRENDER_WIRE_FORCE_COLORS, clear = flags & CRENDER_WIRE_CLEAR;
    if (T < 0 || H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide || !d_color || !d_status ||
        (flags & ~7u) || (T > 0 && !d_tri) || (!force && !line_bgr3) ||
        (force && (!d_col || !d_key || T >= ((int64_t)1 << 30))) || (clear && (!d_z || !d_normal)))
        return fail(CRENDER_EINVAL, "crender_wire_draw: bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CR_HIP(hipMemsetAsync(d_status, 0, sizeof(int32_t), st));
    if (T > 0) {
        hipLaunchKernelGGL(k_wire_check, dim3(grid_for((size_t)T * 3, 2048)), dim3(kThreads), 0, st, d_tri,
                           T * 3, d_status);
        CR_LAUNCH_CHECK("k_wire_check");
    }
    if (clear) {
        hipLaunchKernelGGL(k_wire_clear, dim3(grid_for((size_t)H * W, 4096)), dim3(kThreads), 0, st, d_z, d_color,
                           d_normal, (size_t)H * W, d_status);
        CR_LAUNCH_CHECK("k_wire_clear");
    }
    if (T == 0) return CRENDER_OK;
    const int64_t nseg = T * 3;
    const dim3 grid((unsigned)((nseg + kThreads - 1) / kThreads));
    const int dots = (flags & CRENDER_WIRE_DOTS) ? 1 : 0;
    if (!force) {
        hipLaunchKernelGGL(k_wire<kStoreConst>, grid, dim3(kThreads), 0, st, d_tri, d_col, nseg, dots,
                           line_bgr3[0], line_bgr3[1], line_bgr3[2], d_color, d_key, H, W, d_status);
        CR_LAUNCH_CHECK("k_wire<store>");
        return CRENDER_OK;
    }
    hipLaunchKernelGGL(k_wire<kKeyMax>, grid, dim3(kThreads), 0, st, d_tri, d_col, nseg, dots, 0.0f, 0.0f, 0.0f,
                       d_color, d_key, H, W, d_status);
    CR_LAUNCH_CHECK("k_wire<keymax>");
    hipLaunchKernelGGL(k_wire<kResolve>, grid, dim3(kThreads), 0, st, d_tri, d_col, nseg, dots, 0.0f, 0.0f, 0.0f,
                       d_color, d_key, H, W, d_status);
    CR_LAUNCH_CHECK("k_wire<resolve>");
    return CRENDER_OK;
}

int crender_wire_overlay(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                         const float *P16, const uint8_t *d_edges, const float *line3, const float *fill3, float width,
                         float feather, float opacity, float *d_color, int H, int W, int y0, int y1, unsigned flags,
                         void *stream)
{
    if (!d_winner || !P16 || !line3 || !d_color)
        return fail(CRENDER_EINVAL, "crender_wire_overlay: d_winner, P16, line3 or d_color is NULL");
    if (T < 0) return fail(CRENDER_EINVAL, "crender_wire_overlay: T is negative");
    if (T > 0 && !d_tri) return fail(CRENDER_EINVAL, "crender_wire_overlay: d_tri is NULL with T > 0");
    if (H < 1 || W < 1) return fail(CRENDER_EINVAL, "crender_wire_overlay: H or W is below 1");
    if (y0 < 0 || y1 > H || y0 >= y1) return fail(CRENDER_EINVAL, "crender_wire_overlay: rows outside the frame");
    if (!isfinite(width) || !(width > 0.0f && width <= (float)CRENDER_WIRE_MAX_WIDTH))
        return fail(CRENDER_EINVAL, "crender_wire_overlay: width is not in (0, 64]");
    if (!isfinite(feather) || !(feather > 0.0f && feather <= (float)CRENDER_WIRE_MAX_WIDTH))
        return fail(CRENDER_EINVAL, "crender_wire_overlay: feather is not in (0, 64]");
    if (!(opacity >= 0.0f && opacity <= 1.0f)) return fail(CRENDER_EINVAL, "crender_wire_overlay: opacity is not in [0, 1]");
    bool finite = isfinite(line3[0]) && isfinite(line3[1]) && isfinite(line3[2]);
    if (fill3) finite = finite && isfinite(fill3[0]) && isfinite(fill3[1]) && isfinite(fill3[2]);
    if (!finite) return fail(CRENDER_EINVAL, "crender_wire_overlay: line3 or fill3 is not finite");
    if (flags) return fail(CRENDER_EINVAL, "crender_wire_overlay: unknown flag bits");
    if (T == 0) return CRENDER_OK;
    WireStyle S{};
    for (int j = 0; j < 3; ++j) {
        S.line[j] = line3[j];
        S.fill[j] = fill3 ? fill3[j] : 0.0f;
    }
    S.hi = width * 0.5f + feather * 0.5f;
    S.feather = feather;
    S.opacity = opacity;
    static constexpr decltype(&k_wire_overlay<false>) kernels[2] = {k_wire_overlay<false>, k_wire_overlay<true>};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[fill3 != nullptr], G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner,
                       d_tri, T, d_pos_of, make_proj(P16, W, H), d_edges, S, d_color, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_wire_overlay");
    return CRENDER_OK;
}

}  // extern "C"
