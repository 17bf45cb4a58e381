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
// of the file), a deferred pass of the shape of k_phong_shade, and after it the outline (k_wire_outline): the same
// lines at full width from a neighbourhood pass over the winner plane staged in LDS, of the shape of k_ao_shade.  And
// what the two draw for a view: the contour edges (k_wire_facing, k_wire_contour_mask), classified per frame.  And the
// coverage of boundary pixels from the same staged winners (k_wire_edge_aa, after the outline): geometric anti-aliasing.
// And the edges BEHIND the surface, dashed (k_wire_hidden, after the contour kernels): k_wire's walker over the z plane.
// And that classification kept as vector segments (k_wire_runs, last): maximal runs per edge, compacted in order.
// In sections of their own after the unit's entry points: transparency (k_peel_*: the layer behind a layer by depth key,
// and its blend), depth of field (k_dof_blur: a gather blur by the circle of confusion over the z plane, staged in LDS),
// normal mapping and environment mapping.
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

#include "winner_pass.h"     // WinnerPixel, winner_triangle, pass_grid; the tile frame, tile_grid; frame_checks

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
        const TriXYZ X = winner_triangle(tri, px.t, P);
        const float c[3][3] = {{X.x0, X.y0, X.z0}, {X.x1, X.y1, X.z1}, {X.x2, X.y2, X.z2}};
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

// ---- the outline (crender_wire_outline) -------------------------------------------------------------------------
// The overlay's lines at full width: a pixel also sees the edges of the triangles that won its NEIGHBOURS, so the
// outer half of a silhouette is drawn, on a farther surface or on the background, and a line is not cut where its
// triangle ends.  A neighbourhood pass over the winner plane, of the shape of k_ao_shade (ao.hip), but with a workgroup
// per tile and no loop over tiles (the loop's state cost scalar registers the kernel does not have): a workgroup owns a
// tile of kTile x kTile pixels and stages the VALIDATED winner — the caller's index, or -1 for background, off the
// frame, outside the strip, t >= T or d_pos_of[t] >= T — of the tile plus a halo of radius_px on every side into LDS
// once, with unit-stride loads along rows; a tap is then one ds_read_b32 and needs no second look at T or d_pos_of.
//
// Geometry.  256 work items are 32 x 8 pixels; a wavefront is two rows of 32 and walks the tile's 32 rows in four
// steps of 8.  ds_read_b32 is served in two lane groups of 32 lanes over 32 banks of 4 bytes: a lane group is ONE row
// of 32 consecutive words, so a tap's read — every lane at its own base plus the same offset — is free of bank
// conflicts under any pitch, and the pitch is simply kTile + 2 R: (32 + 2 R)^2 words, 4.6 KB at R = 1, 9.2 KB at
// R = 8, plus one word per staged row that says whether the row holds a winner at all.
//
// Work.  A pixel handles its own winner first, then walks the (2 R + 1)^2 taps, four reads in flight at a time
// (a tap's decision waits for its read: one tap at a time the loop is bound by the latency of the LDS), and skips a
// tap that is -1, its own winner, or one of the four triangles it handled last: a wavefront pays for a candidate
// whenever one of its lanes takes one, and a window that straddles two or three triangles would otherwise take them
// again at every row.  Where triangles are larger than the window nearly every group of four is skipped after its reads.  A new candidate costs the corner gather, the projection (nine divisions) and a division
// and a square root per drawn edge.  The minimum is exact, so the order of the taps does not matter.  A wavefront
// whose two rows' window holds no winner leaves after one read per staged row of it; a workgroup over background alone
// is four such wavefronts.

// The statements "Per candidate" of crender_wire_outline: the distances of (fx, fy) to the drawn edge SEGMENTS of the
// triangle at d_tri[pos], each taken into m if it counts there (`always`, or nearer than zp by the bias).
CR_DEV void outline_candidate(const float *__restrict__ tri, int64_t pos, const ProjConst &P, unsigned mask, float fx,
                              float fy, bool always, float bias, float zp, float &m)
{
    const TriXYZ X = winner_triangle(tri, pos, P);
    const float c[3][3] = {{X.x0, X.y0, X.z0}, {X.x1, X.y1, X.z1}, {X.x2, X.y2, X.z2}};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (!((mask >> e) & 1u)) continue;
        const float *a = c[e], *b = c[(e + 1) % 3];
        const float ex = b[0] - a[0], ey = b[1] - a[1];
        const float px = fx - a[0], py = fy - a[1];
        float s = (px * ex + py * ey) / (ex * ex + ey * ey);
        s = s < 0.0f ? 0.0f : s;                    // (selects: a NaN passes both)
        s = s > 1.0f ? 1.0f : s;
        const float qx = a[0] + s * ex, qy = a[1] + s * ey;
        const float cx = fx - qx, cy = fy - qy;
        const float d = sqrtf(cx * cx + cy * cy);
        const float ze = a[2] + s * (b[2] - a[2]);
        const bool counts = always || (ze - bias) < zp;
        if (counts && d < m) m = d;                 // (a NaN is never taken)
    }
}

// FILL: every covered pixel is stored, over the fill colour; a background pixel, and without FILL every pixel, only
// on a line, over its own colour.
template <bool FILL>
__global__ __launch_bounds__(kThreads) void k_wire_outline(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                            const float *__restrict__ tri, int64_t T,
                                                            const uint32_t *__restrict__ pos_of, ProjConst P,
                                                            const uint8_t *__restrict__ edges, WireStyle S, float bias,
                                                            int R, float *__restrict__ cb, int W, int y0, int y1,
                                                            int tiles_x)
{
    extern __shared__ int32_t s_win[];          // [kTile + 2R][kTile + 2R], then s_row[kTile + 2R]
    const int side = 2 * R + 1, pitch = kTile + 2 * R;
    int32_t *s_row = s_win + pitch * pitch;     // 1 if the staged row holds a winner
    const auto [lane, wave, lx, ly] = tile_lane();
    const auto [x0, ty0] = tile_origin(blockIdx.x, tiles_x, y0);
    // ---- stage the validated winners of the tile and its halo: a wavefront per row, 64 columns at a time
    for (int sy = wave; sy < pitch; sy += kThreads / 64) {
        const int gy = ty0 - R + sy;
        const bool row_in = gy >= y0 && gy < y1;
        bool in_row = false;
        for (int sx = lane; sx < pitch; sx += 64) {
            const int gx = x0 - R + sx;
            int32_t v = -1;
            if (row_in && gx >= 0 && gx < W) {
                const int32_t w = win[(size_t)gy * (size_t)W + (size_t)gx];
                if (w >= 0 && w < T && (!pos_of || pos_of[w] < T)) v = w;
            }
            s_win[sy * pitch + sx] = v;
            in_row |= v >= 0;
        }
        in_row = wave_any(in_row);
        if (lane == 0) s_row[sy] = in_row ? 1 : 0;
    }
    __syncthreads();
    // ---- the tile's pixels, 32 x 8 at a time
#pragma unroll 1
    for (int k = 0; k < kTile / kTileRows; ++k) {
        const int row = ly + k * kTileRows;
        // the staged rows this wavefront's two rows can reach: (row of lane 0) .. + 1 + 2R
        const int first = row - (lane >> 5);
        int reach = 0;
        for (int r = first; r <= first + 1 + 2 * R; ++r) reach |= s_row[r];
        if (!wave_any(reach != 0)) continue;        // a scalar branch: the whole wavefront skips
        const int x = x0 + lx, y = ty0 + row;
        if (!(x < W && y < y1)) continue;
        const size_t pix = (size_t)y * (size_t)W + (size_t)x;
        const int base = (row + R) * pitch + lx + R;
        const int32_t own = s_win[base];
        const float zp = zb[pix];
        const float fx = (float)x, fy = (float)y;
        float m = INFINITY;
        // the pixel's own winner first, then the window row by row, four taps in flight at a time
        if (own >= 0)
            outline_candidate(tri, pos_of ? (int64_t)pos_of[own] : (int64_t)own, P, edges ? edges[own] : 7u, fx, fy, true,
                              bias, zp, m);
        int32_t h0 = -1, h1 = -1, h2 = -1, h3 = -1;     // the four candidates handled last
        for (int dy = -R; dy <= R; ++dy) {
            const int32_t *rp = s_win + (base + dy * pitch - R);
            for (int j = 0; j < side; j += 4) {
                // (a word past the row's end is still inside the allocation, s_row follows the tile, and is not used)
                const int32_t t0 = rp[j], r1 = rp[j + 1], r2 = rp[j + 2], r3 = rp[j + 3];
                const int32_t t1 = j + 1 < side ? r1 : -1, t2 = j + 2 < side ? r2 : -1, t3 = j + 3 < side ? r3 : -1;
                const bool fresh = (t0 >= 0 && t0 != own) || (t1 >= 0 && t1 != own) || (t2 >= 0 && t2 != own) ||
                                   (t3 >= 0 && t3 != own);
                if (!fresh) continue;
#pragma unroll 1
                for (int k = 0; k < 4; ++k) {
                    const int32_t t = k == 0 ? t0 : k == 1 ? t1 : k == 2 ? t2 : t3;
                    if (t < 0 || t == own || t == h0 || t == h1 || t == h2 || t == h3) continue;
                    h3 = h2; h2 = h1; h1 = h0; h0 = t;
                    outline_candidate(tri, pos_of ? (int64_t)pos_of[t] : (int64_t)t, P, edges ? edges[t] : 7u, fx, fy,
                                      own < 0, bias, zp, m);
                }
            }
        }
        float a = (S.hi - m) / S.feather;       // (the overlay's ending, with `own >= 0` beside FILL)
        const bool on = a > 0.0f;
        a = a > 1.0f ? 1.0f : a;
        a = a * S.opacity;
        float *cp = cb + pix * 3;
        if (FILL && own >= 0) {
            const float kk = 1.0f - a;
#pragma unroll
            for (int j = 0; j < 3; ++j) cp[j] = on ? S.fill[j] * kk + S.line[j] * a : S.fill[j];
        } else if (on) {
            const float kk = 1.0f - a;
#pragma unroll
            for (int j = 0; j < 3; ++j) cp[j] = cp[j] * kk + S.line[j] * a;
        }
    }
}

// ---- geometric edge anti-aliasing (crender_wire_edge_aa) --------------------------------------------------------
// The coverage of a boundary pixel from the winner plane: where a pixel's left, right, upper or lower neighbour names
// another triangle, the nearer of the two triangles (by the z plane) has an edge that crosses the line between the two
// pixel centres, the rasterizer's own barycentrics at the two centres say where, and the pixel is blended with the one
// neighbour that reaches farthest into its cell.  The outline's shape at R = 1: a workgroup per tile of 32 x 32 pixels,
// the validated winners of the tile and a halo of one pixel staged in LDS with unit-stride loads (34^2 words), a
// wavefront two rows of 32, so that each of the four taps is a ds_read_b32 without bank conflicts.  The colour plane is
// only read and the result goes to a plane of its own (a pixel reads its neighbours' colours).
//
// Work.  A wavefront none of whose lanes has a differing neighbour copies its 64 colours, 12 bytes a lane at unit
// stride, and that is nearly every wavefront of a frame: a scalar branch.  A lane with a differing neighbour reads z,
// and for each such neighbour gathers and projects the near triangle (nine divisions), takes its barycentrics at both
// centres (six) and up to three exits.  The pixel's own winner is the near triangle in most directions: it is
// projected once per pixel; the neighbour's triangle is kept while the next direction names the same one.

__global__ __launch_bounds__(kThreads) void k_wire_edge_aa(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                            const float *__restrict__ tri, int64_t T,
                                                            const uint32_t *__restrict__ pos_of, ProjConst P,
                                                            const uint8_t *__restrict__ edges, float *__restrict__ ob,
                                                            const float *__restrict__ cb, int W, int y0, int y1,
                                                            int tiles_x)
{
    extern __shared__ int32_t s_win[];          // [kTile + 2][kTile + 2]
    constexpr int pitch = kTile + 2;
    const auto [lane, wave, lx, ly] = tile_lane();
    const auto [x0, ty0] = tile_origin(blockIdx.x, tiles_x, y0);
    // ---- stage the validated winners of the tile and its halo (the outline's rule): a wavefront per row
    for (int sy = wave; sy < pitch; sy += kThreads / 64) {
        const int gy = ty0 - 1 + sy;
        const bool row_in = gy >= y0 && gy < y1;
        if (lane < pitch) {
            const int gx = x0 - 1 + lane;
            int32_t v = -1;
            if (row_in && gx >= 0 && gx < W) {
                const int32_t w = win[(size_t)gy * (size_t)W + (size_t)gx];
                if (w >= 0 && w < T && (!pos_of || pos_of[w] < T)) v = w;
            }
            s_win[sy * pitch + lane] = v;
        }
    }
    __syncthreads();
    // ---- the tile's pixels, 32 x 8 at a time
#pragma unroll 1
    for (int k = 0; k < kTile / kTileRows; ++k) {
        const int row = ly + k * kTileRows;
        const int x = x0 + lx, y = ty0 + row;
        const bool inside = x < W && y < y1;
        const int base = (row + 1) * pitch + lx + 1;
        const int32_t own = s_win[base];
        // a neighbour off the frame or outside the strip is not looked at (its staged word is -1, which is not `own`
        // for a covered pixel)
        // (the four taps are read whatever the pixel is, one ds_read_b32 each, and combined without a branch)
        const int32_t wl = s_win[base - 1], wr = s_win[base + 1], wu = s_win[base - pitch], wd = s_win[base + pitch];
        const bool differs = inside & (((x > 0) & (wl != own)) | ((x + 1 < W) & (wr != own)) | ((y > y0) & (wu != own)) |
                                       ((y + 1 < y1) & (wd != own)));
        const size_t pix = (size_t)y * (size_t)W + (size_t)x;
        float c[3] = {0.0f, 0.0f, 0.0f};
        if (inside) {
            const float *cp = cb + pix * 3;
            c[0] = cp[0]; c[1] = cp[1]; c[2] = cp[2];
        }
        if (!wave_any(differs)) {                   // a scalar branch: the whole wavefront only copies
            if (inside) {
                float *op = ob + pix * 3;
                op[0] = c[0]; op[1] = c[1]; op[2] = c[2];
            }
            continue;
        }
        if (!inside) continue;
        float a = 0.0f;
        size_t qpix = pix;                          // the neighbour the pixel is blended with
        if (differs) {
            const float zp = zb[pix];
            TriXYZ mine = {}, theirs = {};          // the own winner projected, and the neighbour's handled last
            bool have_mine = false;
            int32_t held = -1;
#pragma unroll 1
            for (int d = 0; d < 4; ++d) {           // (-1, 0), (+1, 0), (0, -1), (0, +1)
                const int dx = d == 0 ? -1 : (d == 1 ? 1 : 0), dy = d == 2 ? -1 : (d == 3 ? 1 : 0);
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= W || qy < y0 || qy >= y1) continue;
                const int32_t wq = s_win[base + dy * pitch + dx];
                if (wq == own) continue;
                const size_t at = (size_t)qy * (size_t)W + (size_t)qx;
                bool near_is_q = wq >= 0;
                if (near_is_q && own >= 0) near_is_q = zb[at] < zp;         // (a NaN makes p the near one)
                const int32_t w = near_is_q ? wq : own;
                const bool is_mine = w == own;
                if (is_mine ? !have_mine : w != held) {
                    const TriXYZ t = winner_triangle(tri, pos_of ? (int64_t)pos_of[w] : (int64_t)w, P);
                    if (is_mine) {
                        mine = t;
                        have_mine = true;
                    } else {
                        theirs = t;
                        held = w;
                    }
                }
                const TriXYZ &t = is_mine ? mine : theirs;
                float bn1, bn2, bn3, bf1, bf2, bf3;
                barycentric(t, near_is_q ? qx : x, near_is_q ? qy : y, bn1, bn2, bn3);
                barycentric(t, near_is_q ? x : qx, near_is_q ? y : qy, bf1, bf2, bf3);
                float tmin = INFINITY;
                int ks = 0;
                if (bf1 < 0.0f) {
                    const float tk = bn1 / (bn1 - bf1);
                    if (tk < tmin) { tmin = tk; ks = 1; }                   // (a NaN is never taken)
                }
                if (bf2 < 0.0f) {
                    const float tk = bn2 / (bn2 - bf2);
                    if (tk < tmin) { tmin = tk; ks = 2; }
                }
                if (bf3 < 0.0f) {
                    const float tk = bn3 / (bn3 - bf3);
                    if (tk < tmin) { tmin = tk; ks = 3; }
                }
                if (ks == 0) continue;              // the far pixel lies inside the near triangle
                const int e = ks == 3 ? 0 : ks;     // b1 vanishes on edge 1, b2 on edge 2, b3 on edge 0
                if (edges && !((edges[w] >> e) & 1u)) continue;
                float s = near_is_q ? tmin - 0.5f : 0.5f - tmin;
                s = s > 0.5f ? 0.5f : s;
                if (s > a) {                        // (the first direction wins a tie; a NaN is never taken)
                    a = s;
                    qpix = at;
                }
            }
        }
        float *op = ob + pix * 3;
        if (a == 0.0f) {
            op[0] = c[0]; op[1] = c[1]; op[2] = c[2];
        } else {
            const float *cq = cb + qpix * 3;
            const float kk = 1.0f - a;
#pragma unroll
            for (int j = 0; j < 3; ++j) op[j] = c[j] * kk + cq[j] * a;
        }
    }
}

// ---- the contour edges (crender_wire_contours) ------------------------------------------------------------------
// Which edges the overlay and the outline should draw for THIS view: the edges between a triangle that faces the
// camera and one that faces away, which no classification made once per model can hold.  Two launches over the
// triangles, in the caller's order, a triangle per work item in a grid-stride loop: the first leaves the sign of every
// triangle's projected area in a byte, the second reads the three partners of a triangle from the model's table and
// compares signs.  A sign is computed once and both sides of an edge read the same two bytes, so the two half-edges of
// a contour always agree.  No LDS: a wavefront's 64 triangles, partner rows and mask bytes are contiguous as they are;
// only the three partner signs are gathered, and in a mesh that keeps neighbours near each other they share cache lines.

// The sign of the projected area of the triangle at d_tri[q]: "Phase 1" of crender_wire.h.
__global__ __launch_bounds__(kThreads) void k_wire_facing(const float *__restrict__ tri, int64_t T,
                                                           const uint32_t *__restrict__ pos_of, ProjConst P,
                                                           int8_t *__restrict__ facing)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < T; t += stride) {
        const int64_t q = pos_of ? (int64_t)pos_of[t] : t;
        int f = 0;
        if (q < T) {
            const TriXYZ X = winner_triangle(tri, q, P);    // (the projected z is not used: its divisions are dropped)
            // l03 of raster_math.h's barycentric, in its operations and their order
            const float l01 = X.x1 - X.x2, l02 = X.y1 - X.y2;
            const float A = l01 * (X.y0 - X.y2) - l02 * (X.x0 - X.x2);
            f = A > 0.0f ? 1 : (A < 0.0f ? -1 : 0);        // (a NaN is neither)
        }
        facing[t] = (int8_t)f;
    }
}

// The mask of a triangle from its partners' signs: "Phase 2" of crender_wire.h.
__global__ __launch_bounds__(kThreads) void k_wire_contour_mask(const int32_t *__restrict__ partners,
                                                                 const uint8_t *__restrict__ fixed,
                                                                 const int8_t *__restrict__ facing, int64_t T, int borders,
                                                                 uint8_t *__restrict__ edges)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < T; t += stride) {
        unsigned bits = fixed ? (fixed[t] & 7u) : 0u;
        const int mine = facing[t];
        const int32_t *row = partners + t * 3;
        const int32_t v0 = row[0], v1 = row[1], v2 = row[2];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int32_t v = e == 0 ? v0 : e == 1 ? v1 : v2;
            bool on = borders && (v == -1 || v == -2);
            const int64_t p = (int64_t)(v >> 1);
            if (v >= 0 && p < T)                       // anything else is "no partner": never an index
                on = mine * (int)facing[p] == ((v & 1) ? 1 : -1);
            bits |= on ? (1u << e) : 0u;
        }
        edges[t] = (uint8_t)bits;
    }
}

// ---- the hidden lines (crender_wire_hidden) ---------------------------------------------------------------------
// The edges BEHIND the surface, dashed: what no pass over the winner plane can draw, since a hidden edge belongs to
// triangles that won nothing where it runs.  The shape of k_wire: one workgroup per 256 half-edges (segment s = 3 i + e,
// i in the caller's order), each work item projects, rounds and clips its own segment with seg_setup, the workgroup
// scans the counts and deals the candidate pixels one per work item.  A step compares the edge's depth, interpolated
// along the major axis (projected z is affine on the screen), with the z plane.  Two launches over a uint32 key plane,
// zero before and after: the first marks a visible step with 2 and a drawn hidden step with 1 by atomicMax, the second
// walks the same candidates again and the one walker that takes a 1 out of a pixel blends the line's colour into it.
// The result is a function of the set of marked pixels.  Per-segment LDS: the Seg's six words, the offset, za and
// zb - za: 9.2 KB per workgroup, static.

enum { kHiddenMark = 0, kHiddenResolve = 1 };

// The line and the test of a call.
struct HiddenStyle {
    float line[3];
    float opacity, bias;
    int on, period;                          // dash_on, dash_on + dash_off
    int use_winner;
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_wire_hidden(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                           const float *__restrict__ tri, int64_t T,
                                                           const uint32_t *__restrict__ pos_of, ProjConst P,
                                                           const uint8_t *__restrict__ edges, int64_t nseg, HiddenStyle S,
                                                           uint32_t *__restrict__ key, float *__restrict__ cb, int H, int W,
                                                           int y0, int y1)
{
    __shared__ int s_a1[kThreads], s_b1[kThreads], s_el[kThreads], s_es[kThreads], s_t0[kThreads],
        s_sg[kThreads];
    __shared__ float s_za[kThreads], s_dz[kThreads];
    __shared__ uint32_t s_off[kThreads];
    __shared__ uint32_t s_wave[kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * kThreads;
    const int64_t seg = first + tid;
    uint32_t cnt = 0;
    Seg s = {0, 0, 0, 0, 0, 0};
    float za = 0.0f, dz = 0.0f;
    if (seg < nseg) {
        const int64_t i = seg / 3;
        const int e = (int)(seg - 3 * i);
        const unsigned mask = edges ? edges[i] : 7u;            // the caller's order, whatever pos_of says
        const int64_t pos = pos_of ? (int64_t)pos_of[i] : i;
        if (((mask >> e) & 1u) && pos < T) {
            float raw[3][3];
            const TriXYZ X = winner_triangle(tri, pos, P, raw);
            // corner e and corner (e + 1) % 3, by selects (an index would put the corners into scratch)
            float xa = e == 0 ? X.x0 : e == 1 ? X.x1 : X.x2, ya = e == 0 ? X.y0 : e == 1 ? X.y1 : X.y2;
            float pza = e == 0 ? X.z0 : e == 1 ? X.z1 : X.z2;
            float xb = e == 0 ? X.x1 : e == 1 ? X.x2 : X.x0, yb = e == 0 ? X.y1 : e == 1 ? X.y2 : X.y0;
            float pzb = e == 0 ? X.z1 : e == 1 ? X.z2 : X.z0;
            const float rza = e == 0 ? raw[0][2] : e == 1 ? raw[1][2] : raw[2][2];
            const float rzb = e == 0 ? raw[1][2] : e == 1 ? raw[2][2] : raw[0][2];
            // in front of the camera (a NaN fails), and in k_wire_check's domain
            if (rza > 0.0f && rzb > 0.0f && fabsf(xa) < kDomain && fabsf(ya) < kDomain && fabsf(xb) < kDomain &&
                fabsf(yb) < kDomain) {
                int ax = (int)rintf(xa), ay = (int)rintf(ya), bx = (int)rintf(xb), by = (int)rintf(yb);
                // from the end whose (y, x) is smaller: both half-edges of an edge then walk the same pixels
                if (by < ay || (by == ay && bx < ax)) {
                    int ti = ax; ax = bx; bx = ti;
                    ti = ay; ay = by; by = ti;
                    const float tf = pza; pza = pzb; pzb = tf;
                }
                cnt = seg_setup(ax, ay, bx, by, W, H, s);
                za = pza;
                dz = pzb - pza;
            }
        }
    }
    s_a1[tid] = s.a1; s_b1[tid] = s.b1; s_el[tid] = s.el; s_es[tid] = s.es; s_t0[tid] = s.t0; s_sg[tid] = s.sg;
    s_za[tid] = za; s_dz[tid] = dz;
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
        const int64_t t = (int64_t)g.t0 + (p - s_off[j]);
        int x, y;
        seg_pixel(g, t, x, y);
        if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) continue;   // (clipped above; kept as a guard)
        if (y < y0 || y >= y1) continue;
        const size_t pix = (size_t)y * W + x;
        if (MODE == kHiddenMark) {
            const float lam = g.el ? (float)t / (float)g.el : 0.0f;
            const float ze = s_za[j] + s_dz[j] * lam;
            bool hidden = zb[pix] < ze - S.bias;                // (false for every NaN; the background's 1e6 never hides)
            if (hidden && S.use_winner && (int64_t)win[pix] == (first + j) / 3) hidden = false;
            if (!hidden) {
                atomicMax(key + pix, 2u);
            } else {
                const int c = (g.sg & 1) ? x : y;               // on the frame: never negative
                if (c % S.period < S.on) atomicMax(key + pix, 1u);
            }
        } else if (atomicExch(key + pix, 0u) == 1u) {              // (one walker per pixel gets the 1)
            float *cp = cb + pix * 3;
            const float k = 1.0f - S.opacity;
#pragma unroll
            for (int c = 0; c < 3; ++c) cp[c] = cp[c] * k + S.line[c] * S.opacity;
        }
    }
}

// The line of an overlay or outline call: its window, then (after what only the outline checks) its colours and the WireStyle.
int wire_window(const char *entry, float width, float feather, float opacity)
{
    if (!isfinite(width) || !(width > 0.0f && width <= (float)CRENDER_WIRE_MAX_WIDTH))
        return arg_error(entry, "width is not in (0, 64]");
    if (!isfinite(feather) || !(feather > 0.0f && feather <= (float)CRENDER_WIRE_MAX_WIDTH))
        return arg_error(entry, "feather is not in (0, 64]");
    return (opacity >= 0.0f && opacity <= 1.0f) ? CRENDER_OK : arg_error(entry, "opacity is not in [0, 1]");
}

int wire_style(const char *entry, const float *line3, const float *fill3, float width, float feather, float opacity, WireStyle &S)
{
    bool finite = isfinite(line3[0]) && isfinite(line3[1]) && isfinite(line3[2]);
    if (fill3) finite = finite && isfinite(fill3[0]) && isfinite(fill3[1]) && isfinite(fill3[2]);
    if (!finite) return arg_error(entry, "line3 or fill3 is not finite");
    for (int j = 0; j < 3; ++j) {
        S.line[j] = line3[j];
        S.fill[j] = fill3 ? fill3[j] : 0.0f;
    }
    S.hi = width * 0.5f + feather * 0.5f;
    S.feather = feather;
    S.opacity = opacity;
    return CRENDER_OK;
}

// ---- the drawing as vectors (crender_wire_runs_count, crender_wire_runs_emit) -----------------------------------
// The hidden pass's classification KEPT: k_wire_hidden's shape — a workgroup per 256 half-edges, each work item sets its
// own segment up, the workgroup scans the counts and deals the candidate steps one per work item, 256 at a time — but a
// step's class (hidden 1, visible 2, off the rows 0) goes into maximal RUNS per segment instead of a key plane.  The order
// of the candidates p within a workgroup is the order (segment, step), so a run's rank in its group is the number of run
// starts at candidates before it, and the k-th start and the k-th end of a group are the same run: the lane that finds a
// start stores (s, t0, class) and the first point into slot k, the lane that finds an end stores t1 and the second point
// into slot k, and nobody walks a run.  A lane looks at ONE neighbour, the candidate before its own, whose class and
// segment it reads from LDS (the last lane's are carried to the next trip): candidate p starts a run if its class is not
// 0 and the pair (segment, class) before it differs, and it ENDS the run of candidate p - 1 if that one's class is not 0
// and the pair differs.  One candidate beyond the last closes the group's last run.  The ranks are a ballot and a count
// of the lanes below per wavefront, the wavefronts' totals through LDS, and two running bases across the trips (a run may
// start in one trip and end in a later one).  No atomics: a slot is a function of the inputs alone.
// Per-segment LDS: k_wire_hidden's nine words, the partner's triangle, and for the emit the four unrounded coordinates.

enum { kRunsCount = 0, kRunsEmit = 1 };

// How many lanes below this one have `flag`, and how many of the wavefront: a ballot and its counts.
CR_DEV uint32_t wave_rank(bool flag, uint32_t &total)
{
    const uint64_t b = __builtin_amdgcn_ballot_w64(flag);
    total = (uint32_t)__popcll(b);
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// A point of a run: x(u) = xa (1 - u) + xb u, which gives the ends back bit for bit at u = 0 and u = 1.
CR_DEV float run_lerp(float a, float b, float u)
{
    return a * (1.0f - u) + b * u;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_wire_runs(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                         const float *__restrict__ tri, int64_t T,
                                                         const uint32_t *__restrict__ pos_of, ProjConst P,
                                                         const uint8_t *__restrict__ edges,
                                                         const int32_t *__restrict__ partners, int64_t nseg, float bias,
                                                         int use_winner, uint32_t *__restrict__ counts,
                                                         const int64_t *__restrict__ offsets, int64_t N,
                                                         int32_t *__restrict__ runs, float *__restrict__ ends, int H, int W,
                                                         int y0, int y1)
{
    constexpr bool EMIT = MODE == kRunsEmit;
    constexpr int kEnds = EMIT ? kThreads : 1;
    __shared__ int s_a1[kThreads], s_b1[kThreads], s_el[kThreads], s_es[kThreads], s_t0[kThreads],
        s_sg[kThreads];
    __shared__ float s_za[kThreads], s_dz[kThreads];
    __shared__ int32_t s_partner[kThreads];             // the triangle across the edge, or -1
    __shared__ float s_xa[kEnds], s_ya[kEnds], s_xb[kEnds], s_yb[kEnds];      // the unrounded ends, in walking order
    __shared__ uint32_t s_off[kThreads];
    __shared__ uint32_t s_wave[kThreads / 64];
    __shared__ uint32_t s_prev[kThreads + 1];           // class | (segment + 1) << 2 of the candidate before each lane's
    __shared__ uint32_t s_starts[kThreads / 64], s_ends[kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * kThreads;
    const int64_t seg = first + tid;
    uint32_t cnt = 0;
    Seg s = {0, 0, 0, 0, 0, 0};
    float za = 0.0f, dz = 0.0f;
    float exa = 0.0f, eya = 0.0f, exb = 0.0f, eyb = 0.0f;
    int32_t partner = -1;
    if (seg < nseg) {
        const int64_t i = seg / 3;
        const int e = (int)(seg - 3 * i);
        const unsigned mask = edges ? edges[i] : 7u;            // the caller's order, whatever pos_of says
        const int64_t pos = pos_of ? (int64_t)pos_of[i] : i;
        if (((mask >> e) & 1u) && pos < T) {
            float raw[3][3];
            const TriXYZ X = winner_triangle(tri, pos, P, raw);
            // corner e and corner (e + 1) % 3, by selects (k_wire_hidden's statements)
            float xa = e == 0 ? X.x0 : e == 1 ? X.x1 : X.x2, ya = e == 0 ? X.y0 : e == 1 ? X.y1 : X.y2;
            float pza = e == 0 ? X.z0 : e == 1 ? X.z1 : X.z2;
            float xb = e == 0 ? X.x1 : e == 1 ? X.x2 : X.x0, yb = e == 0 ? X.y1 : e == 1 ? X.y2 : X.y0;
            float pzb = e == 0 ? X.z1 : e == 1 ? X.z2 : X.z0;
            const float rza = e == 0 ? raw[0][2] : e == 1 ? raw[1][2] : raw[2][2];
            const float rzb = e == 0 ? raw[1][2] : e == 1 ? raw[2][2] : raw[0][2];
            if (rza > 0.0f && rzb > 0.0f && fabsf(xa) < kDomain && fabsf(ya) < kDomain && fabsf(xb) < kDomain &&
                fabsf(yb) < kDomain) {
                int ax = (int)rintf(xa), ay = (int)rintf(ya), bx = (int)rintf(xb), by = (int)rintf(yb);
                if (by < ay || (by == ay && bx < ax)) {         // from the end whose (y, x) is smaller
                    int ti = ax; ax = bx; bx = ti;
                    ti = ay; ay = by; by = ti;
                    float tf = pza; pza = pzb; pzb = tf;
                    tf = xa; xa = xb; xb = tf;
                    tf = ya; ya = yb; yb = tf;
                }
                cnt = seg_setup(ax, ay, bx, by, W, H, s);
                za = pza;
                dz = pzb - pza;
                exa = xa; eya = ya; exb = xb; eyb = yb;
                if (use_winner && partners) {
                    const int32_t v = partners[i * 3 + e];
                    if (v >= 0) partner = v >> 1;
                }
            }
        }
    }
    s_a1[tid] = s.a1; s_b1[tid] = s.b1; s_el[tid] = s.el; s_es[tid] = s.es; s_t0[tid] = s.t0; s_sg[tid] = s.sg;
    s_za[tid] = za; s_dz[tid] = dz;
    s_partner[tid] = partner;
    if (EMIT) {
        s_xa[tid] = exa; s_ya[tid] = eya; s_xb[tid] = exb; s_yb[tid] = eyb;
    }
    if (tid == 0) s_prev[0] = 0u;                               // nothing lies before the group's first candidate
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
    int64_t slot0 = 0, limit = 0;                               // the group's first slot, and the first that is not its own
    if (EMIT) {
        slot0 = offsets[blockIdx.x];
        limit = blockIdx.x + 1u < gridDim.x ? offsets[blockIdx.x + 1u] : N;
        limit = limit < N ? limit : N;
    }
    uint32_t nstart = 0, nend = 0;                              // the starts and ends of the trips so far (uniform)
    // candidates 0 .. total - 1, and one beyond them, which ends the last run
    for (uint32_t c0 = 0; c0 <= total; c0 += kThreads) {
        const uint32_t p = c0 + tid;
        uint32_t cls = 0;
        int j = -1, t = 0;
        if (p < total) {
            // the last segment whose first candidate is at or before p holds p (empty ones share the next offset)
            j = 0;
#pragma unroll
            for (int step = kThreads / 2; step; step >>= 1)
                if (s_off[j + step] <= p) j += step;
            const Seg g = {s_a1[j], s_b1[j], s_el[j], s_es[j], s_t0[j], s_sg[j]};
            t = g.t0 + (int)(p - s_off[j]);
            int x, y;
            seg_pixel(g, (int64_t)t, x, y);
            if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H && y >= y0 && y < y1) {
                const size_t pix = (size_t)y * W + x;
                const float lam = g.el ? (float)t / (float)g.el : 0.0f;
                const float ze = s_za[j] + s_dz[j] * lam;
                bool hidden = zb[pix] < ze - bias;              // (false for every NaN)
                if (hidden && use_winner) {
                    const int64_t w = (int64_t)win[pix];
                    const int32_t q = s_partner[j];
                    if (w == (first + j) / 3 || (q >= 0 && w == (int64_t)q)) hidden = false;
                }
                cls = hidden ? 1u : 2u;
            }
        }
        const uint32_t mine = cls | ((uint32_t)(j + 1) << 2);
        s_prev[tid + 1] = mine;
        __syncthreads();
        const uint32_t prev = s_prev[tid];
        const bool differs = prev != mine;                      // another segment, or another class
        const bool start = cls != 0u && differs;
        const bool end = (prev & 3u) != 0u && differs;          // of the run that holds candidate p - 1
        uint32_t wave_starts, wave_ends;
        const uint32_t rs = wave_rank(start, wave_starts), re = wave_rank(end, wave_ends);
        if ((tid & 63) == 0) {
            s_starts[tid >> 6] = wave_starts;
            s_ends[tid >> 6] = wave_ends;
        }
        __syncthreads();
        uint32_t ks = nstart + rs, ke = nend + re;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            ks += w < (tid >> 6) ? s_starts[w] : 0u;
            ke += w < (tid >> 6) ? s_ends[w] : 0u;
            nstart += s_starts[w];
            nend += s_ends[w];
        }
        if (EMIT) {
            if (start) {
                const int64_t slot = slot0 + (int64_t)ks;
                if (slot >= 0 && slot < limit) {
                    const int el = s_el[j];
                    const float u = el ? fmaxf((float)t - 0.5f, 0.0f) / (float)el : 0.0f;
                    int32_t *r = runs + slot * 4;
                    float *q = ends + slot * 4;
                    r[0] = (int32_t)(first + j);
                    r[1] = t;
                    r[3] = (int32_t)cls;
                    q[0] = run_lerp(s_xa[j], s_xb[j], u);
                    q[1] = run_lerp(s_ya[j], s_yb[j], u);
                }
            }
            if (end) {
                const int jp = (int)(prev >> 2) - 1;            // candidate p - 1: its segment, and its step
                const int tp = s_t0[jp] + (int)(p - 1u - s_off[jp]);
                const int64_t slot = slot0 + (int64_t)ke;
                if (slot >= 0 && slot < limit) {
                    const int el = s_el[jp];
                    const float u = el ? fminf((float)tp + 0.5f, (float)el) / (float)el : 1.0f;
                    runs[slot * 4 + 2] = tp;
                    float *q = ends + slot * 4;
                    q[2] = run_lerp(s_xa[jp], s_xb[jp], u);
                    q[3] = run_lerp(s_ya[jp], s_yb[jp], u);
                }
            }
        }
        if (tid == kThreads - 1) s_prev[0] = mine;              // (every lane has read its word: the barrier above)
    }
    if (!EMIT && tid == 0) counts[blockIdx.x] = nstart;
}

// The checks the two entries share, in the header's order; `nulls` names the pointers that were found NULL.
int runs_checks(const char *entry, bool null_arg, const char *nulls, int64_t T, const float *d_tri, int H, int W, int y0,
                int y1, float depth_bias, unsigned flags, int64_t N)
{
    if (null_arg) return arg_error(entry, nulls);
    if (int rc = frame_checks(entry, T, d_tri, H, W)) return rc;
    if (int rc = rows_check(entry, H, y0, y1)) return rc;
    if (H > kMaxSide || W > kMaxSide) return arg_error(entry, "H or W is above 2^20");
    if (!isfinite(depth_bias)) return arg_error(entry, "depth_bias is not finite");
    if (flags & ~CRENDER_WIRE_RUNS_USE_WINNER) return arg_error(entry, "unknown flag bits");
    if (N < 0) return arg_error(entry, "N is negative");
    if (T > (int64_t)0x7FFFFFFF / 3) return arg_error(entry, "T is too large");        // 3 T segments in an int32
    return CRENDER_OK;
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
    const char *const E = "crender_wire_overlay";
    if (!d_winner || !P16 || !line3 || !d_color) return arg_error(E, "d_winner, P16, line3 or d_color is NULL");
    if (int rc = frame_checks(E, T, d_tri, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    WireStyle S{};
    if (int rc = wire_window(E, width, feather, opacity)) return rc;
    if (int rc = wire_style(E, line3, fill3, width, feather, opacity, S)) return rc;
    if (flags) return arg_error(E, "unknown flag bits");
    if (T == 0) return CRENDER_OK;
    static constexpr decltype(&k_wire_overlay<false>) kernels[2] = {k_wire_overlay<false>, k_wire_overlay<true>};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[fill3 != nullptr], G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner,
                       d_tri, T, d_pos_of, make_proj(P16, W, H), d_edges, S, d_color, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_wire_overlay");
    return CRENDER_OK;
}

int crender_wire_outline(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T,
                         const uint32_t *d_pos_of, const float *P16, const uint8_t *d_edges, const float *line3,
                         const float *fill3, float width, float feather, float opacity, float depth_bias, int radius_px,
                         float *d_color, int H, int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_wire_outline";
    if (!d_winner || !d_z || !P16 || !line3 || !d_color) return arg_error(E, "d_winner, d_z, P16, line3 or d_color is NULL");
    if (int rc = frame_checks(E, T, d_tri, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    WireStyle S{};
    if (int rc = wire_window(E, width, feather, opacity)) return rc;
    if (!isfinite(depth_bias)) return arg_error(E, "depth_bias is not finite");
    if (radius_px < 0 || radius_px > CRENDER_WIRE_OUTLINE_MAX_RADIUS) return arg_error(E, "radius_px is not 0 .. 8");
    if (int rc = wire_style(E, line3, fill3, width, feather, opacity, S)) return rc;
    if (flags) return arg_error(E, "unknown flag bits");
    if (T == 0) return CRENDER_OK;
    int tiles_x, tiles;
    if (int rc = tile_grid(E, W, y0, y1, tiles_x, tiles)) return rc;
    static constexpr decltype(&k_wire_outline<false>) kernels[2] = {k_wire_outline<false>, k_wire_outline<true>};
    hipLaunchKernelGGL(kernels[fill3 != nullptr], dim3((unsigned)tiles), dim3(kThreads),
                       tile_lds_bytes(radius_px, kTile + 2 * radius_px), static_cast<hipStream_t>(stream), d_winner, d_z,
                       d_tri, T, d_pos_of, make_proj(P16, W, H), d_edges, S, depth_bias, radius_px, d_color, W, y0, y1,
                       tiles_x);
    CR_LAUNCH_CHECK("k_wire_outline");
    return CRENDER_OK;
}

int crender_wire_edge_aa(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                         const float *P16, const uint8_t *d_edges, float *d_out, const float *d_color, int H, int W,
                         int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_wire_edge_aa";
    if (!d_winner || !d_z || !P16 || !d_out || !d_color) return arg_error(E, "d_winner, d_z, P16, d_out or d_color is NULL");
    if (int rc = frame_checks(E, T, d_tri, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags) return arg_error(E, "unknown flag bits");
    if (d_out == d_color) return arg_error(E, "d_out is d_color (the pass cannot run in place)");
    int tiles_x, tiles;
    if (int rc = tile_grid(E, W, y0, y1, tiles_x, tiles)) return rc;
    // (T == 0: every winner is invalid and every wavefront copies)
    hipLaunchKernelGGL(k_wire_edge_aa, dim3((unsigned)tiles), dim3(kThreads), tile_lds_bytes(1),
                       static_cast<hipStream_t>(stream), d_winner, d_z, d_tri, T, d_pos_of, make_proj(P16, W, H), d_edges,
                       d_out, d_color, W, y0, y1, tiles_x);
    CR_LAUNCH_CHECK("k_wire_edge_aa");
    return CRENDER_OK;
}

int crender_wire_contours(const float *d_tri, int64_t T, const uint32_t *d_pos_of, const float *P16,
                          const int32_t *d_partners, const uint8_t *d_static, int8_t *d_facing, uint8_t *d_edges, int H,
                          int W, unsigned flags, void *stream)
{
    const char *const E = "crender_wire_contours";
    if (!P16 || !d_partners || !d_facing || !d_edges) return arg_error(E, "P16, d_partners, d_facing or d_edges is NULL");
    if (int rc = frame_checks(E, T, d_tri, H, W)) return rc;
    if (flags & ~CRENDER_WIRE_CONTOUR_BORDERS) return arg_error(E, "unknown flag bits");
    if (T == 0) return CRENDER_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((size_t)T, 16384));
    hipLaunchKernelGGL(k_wire_facing, grid, dim3(kThreads), 0, st, d_tri, T, d_pos_of, make_proj(P16, W, H), d_facing);
    CR_LAUNCH_CHECK("k_wire_facing");
    hipLaunchKernelGGL(k_wire_contour_mask, grid, dim3(kThreads), 0, st, d_partners, d_static, d_facing, T,
                       (flags & CRENDER_WIRE_CONTOUR_BORDERS) ? 1 : 0, d_edges);
    CR_LAUNCH_CHECK("k_wire_contour_mask");
    return CRENDER_OK;
}

int crender_wire_hidden(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                        const float *P16, const uint8_t *d_edges, const float *line3, float opacity, int dash_on,
                        int dash_off, float depth_bias, uint32_t *d_key, float *d_color, int H, int W, int y0, int y1,
                        unsigned flags, void *stream)
{
    const char *const E = "crender_wire_hidden";
    if (!d_winner || !d_z || !P16 || !line3 || !d_key || !d_color)
        return arg_error(E, "d_winner, d_z, P16, line3, d_key or d_color is NULL");
    if (int rc = frame_checks(E, T, d_tri, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (H > kMaxSide || W > kMaxSide) return arg_error(E, "H or W is above 2^20");      // (crender_wire_key_bytes' bound)
    if (!(opacity >= 0.0f && opacity <= 1.0f)) return arg_error(E, "opacity is not in [0, 1]");
    if (!(isfinite(line3[0]) && isfinite(line3[1]) && isfinite(line3[2]))) return arg_error(E, "line3 is not finite");
    if (dash_on < 1 || dash_on > CRENDER_WIRE_MAX_DASH || dash_off < 0 || dash_off > CRENDER_WIRE_MAX_DASH)
        return arg_error(E, "dash_on is not 1 .. 64 or dash_off is not 0 .. 64");
    if (!isfinite(depth_bias)) return arg_error(E, "depth_bias is not finite");
    if (flags & ~CRENDER_WIRE_HIDDEN_USE_WINNER) return arg_error(E, "unknown flag bits");
    if (T > ((int64_t)0x7FFFFFFF * kThreads) / 3) return arg_error(E, "T is too large");   // 3 T segments, 256 to a workgroup
    if (T == 0) return CRENDER_OK;
    const HiddenStyle S = {{line3[0], line3[1], line3[2]}, opacity, depth_bias, dash_on, dash_on + dash_off,
                           (flags & CRENDER_WIRE_HIDDEN_USE_WINNER) ? 1 : 0};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t nseg = T * 3;
    const dim3 grid((unsigned)((nseg + kThreads - 1) / kThreads));
    const ProjConst P = make_proj(P16, W, H);
    hipLaunchKernelGGL(k_wire_hidden<kHiddenMark>, grid, dim3(kThreads), 0, st, d_winner, d_z, d_tri, T, d_pos_of, P, d_edges,
                       nseg, S, d_key, d_color, H, W, y0, y1);
    CR_LAUNCH_CHECK("k_wire_hidden<mark>");
    hipLaunchKernelGGL(k_wire_hidden<kHiddenResolve>, grid, dim3(kThreads), 0, st, d_winner, d_z, d_tri, T, d_pos_of, P,
                       d_edges, nseg, S, d_key, d_color, H, W, y0, y1);
    CR_LAUNCH_CHECK("k_wire_hidden<resolve>");
    return CRENDER_OK;
}

int64_t crender_wire_runs_groups(int64_t T)
{
    if (T < 0 || T > (int64_t)0x7FFFFFFF / 3) return -1;
    return (T * 3 + CRENDER_WIRE_RUNS_GROUP - 1) / CRENDER_WIRE_RUNS_GROUP;
}

int crender_wire_runs_count(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                            const float *P16, const uint8_t *d_edges, const int32_t *d_partners, float depth_bias,
                            uint32_t *d_counts, int H, int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_wire_runs_count";
    if (int rc = runs_checks(E, !d_winner || !d_z || !P16 || !d_counts, "d_winner, d_z, P16 or d_counts is NULL", T, d_tri, H,
                             W, y0, y1, depth_bias, flags, 0))
        return rc;
    if (T == 0) return CRENDER_OK;
    static_assert(CRENDER_WIRE_RUNS_GROUP == kThreads, "a group is a workgroup's segments");
    const int64_t nseg = T * 3;
    hipLaunchKernelGGL(k_wire_runs<kRunsCount>, dim3((unsigned)crender_wire_runs_groups(T)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_winner, d_z, d_tri, T, d_pos_of, make_proj(P16, W, H), d_edges,
                       d_partners, nseg, depth_bias, (flags & CRENDER_WIRE_RUNS_USE_WINNER) ? 1 : 0, d_counts,
                       (const int64_t *)nullptr, (int64_t)0, (int32_t *)nullptr, (float *)nullptr, H, W, y0, y1);
    CR_LAUNCH_CHECK("k_wire_runs<count>");
    return CRENDER_OK;
}

int crender_wire_runs_emit(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                           const float *P16, const uint8_t *d_edges, const int32_t *d_partners, float depth_bias,
                           const int64_t *d_offsets, int64_t N, int32_t *d_runs, float *d_ends, int H, int W, int y0, int y1,
                           unsigned flags, void *stream)
{
    const char *const E = "crender_wire_runs_emit";
    if (int rc = runs_checks(E, !d_winner || !d_z || !P16 || !d_offsets || !d_runs || !d_ends,
                             "d_winner, d_z, P16, d_offsets, d_runs or d_ends is NULL", T, d_tri, H, W, y0, y1, depth_bias,
                             flags, N))
        return rc;
    if (T == 0 || N == 0) return CRENDER_OK;
    const int64_t nseg = T * 3;
    hipLaunchKernelGGL(k_wire_runs<kRunsEmit>, dim3((unsigned)crender_wire_runs_groups(T)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_winner, d_z, d_tri, T, d_pos_of, make_proj(P16, W, H), d_edges,
                       d_partners, nseg, depth_bias, (flags & CRENDER_WIRE_RUNS_USE_WINNER) ? 1 : 0, (uint32_t *)nullptr,
                       d_offsets, N, d_runs, d_ends, H, W, y0, y1);
    CR_LAUNCH_CHECK("k_wire_runs<emit>");
    return CRENDER_OK;
}

}  // extern "C"

// ---- bloom (crender_bloom) ----
// A glow around what is brighter than a threshold, and the curve that brings the range back into 0 .. 255: a post-process
// over ANY float32 image [H][W][3], not over the winner plane.  Separable: the bright values are blurred along the rows
// into a scratch plane hb (k_bloom_rows), hb is blurred along the columns, composited over the source, tone mapped,
// clamped and stored (k_bloom_finish): 2 (2 R + 1) taps a pixel where a gather walks (2 R + 1)^2.
//
// Geometry.  k_ao_shade's (ao.hip): a workgroup of 256 per tile of kTile x kTile pixels, looping over tiles; 256 work
// items are 32 x 8 pixels, a wavefront two rows of 32.  A kernel stages what its taps read once into THREE planes of
// LDS, one per channel, so that a tap is one ds_read_b32 per channel at the lane's base plus a wave-uniform offset and a
// lane group reads 32 consecutive words: free of bank conflicts.  k_bloom_rows stages 32 rows x (32 + 2 R) columns of
// bright values (the bright pass is made as they are staged: one division per staged bright pixel), k_bloom_finish
// (32 + 2 R) rows x 32 columns of hb: 3 * 32 * (32 + 2 R) words each, 13 056 B at R = 1, 18 432 B at 8, 36 864 B at 32.
// A staged value off the frame or outside the strip is +0.
//
// Work.  The taps are walked in the contract's order, -R .. R, four at a time so that twelve reads are in flight, each
// tap one multiply and one add per channel; the weights are read from the kernel arguments at a wave-uniform index.
// Dark work is skipped, which cannot change a bit (finite weights: a sum of products with +-0 from +0 is +0): in
// k_bloom_rows a wavefront stages the rows it walks, two at a time, and walks a pair only if one of its staged values
// is not +-0 (a scalar branch); in k_bloom_finish the workgroup ORs what its wavefronts staged through four words of
// LDS, and a dark tile goes straight to the copy of rule 4 and the tone stage.

namespace {

constexpr int kBloomMaxGrid = 2048;          // workgroups of a launch: 8 per CU; the kernels loop over the other tiles
constexpr int kBloomTaps = 4;                // taps whose reads are in flight together

// The constants of a call; w[k] is the weight of the taps at distance k.
struct BloomParams {
    float threshold, intensity, exposure, inv255, iw2, clamp;
    int R, H, tone, reinhard, gamma2, flip;
    float w[CRENDER_BLOOM_MAX_RADIUS + 1];
};

__device__ inline bool bloom_lit(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) != 0u; }      // not +-0

// The 2 R + 1 taps of one pixel along one direction: plane words base, base + step, ...; the sums start from +0.
__device__ inline void bloom_walk(const float *p0, const float *p1, const float *p2, int base, int step,
                                  const BloomParams &A, float &a0, float &a1, float &a2)
{
    const int R = A.R, n = 2 * R + 1;
    int t = 0;
    for (; t + kBloomTaps <= n; t += kBloomTaps) {
        float v0[kBloomTaps], v1[kBloomTaps], v2[kBloomTaps];
#pragma unroll
        for (int j = 0; j < kBloomTaps; ++j) {
            const int at = base + (t + j) * step;
            v0[j] = p0[at]; v1[j] = p1[at]; v2[j] = p2[at];
        }
#pragma unroll
        for (int j = 0; j < kBloomTaps; ++j) {
            const int d = t + j - R;
            const float w = A.w[d < 0 ? -d : d];
            a0 = a0 + w * v0[j];
            a1 = a1 + w * v1[j];
            a2 = a2 + w * v2[j];
        }
    }
    for (; t < n; ++t) {                        // the last one or three taps
        const int at = base + t * step, d = t - R;
        const float w = A.w[d < 0 ? -d : d];
        a0 = a0 + w * p0[at];
        a1 = a1 + w * p1[at];
        a2 = a2 + w * p2[at];
    }
}

__global__ __launch_bounds__(kThreads) void k_bloom_rows(const float *__restrict__ src, BloomParams A,
                                                          float *__restrict__ hb, int W, int y0, int y1, int tiles_x,
                                                          int ntiles)
{
    extern __shared__ float s_bloom[];          // the bright r, g, b: [kTile][kTile + 2R] each
    const int R = A.R, pitch = kTile + 2 * R, plane = kTile * pitch;
    float *const s0 = s_bloom, *const s1 = s_bloom + plane, *const s2 = s_bloom + 2 * plane;
    const auto [lane, wave, lx, ly] = tile_lane();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [x0, ty0] = tile_origin(tile, tiles_x, y0);
        // ---- the bright pass into LDS: a wavefront stages the rows it walks, 2 wave, 2 wave + 1 (+ 8 k)
        unsigned lit = 0;                       // bit k: a value staged for the k-th pair of rows is not +-0
#pragma unroll
        for (int k = 0; k < kTile / kTileRows; ++k) {
            bool some = false;
            for (int j = 0; j < 2; ++j) {
                const int sy = 2 * wave + j + k * kTileRows, gy = ty0 + sy;
                for (int sx = lane; sx < pitch; sx += 64) {
                    const int gx = x0 - R + sx;
                    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
                    if (gy < y1 && gx >= 0 && gx < W) {
                        const float *cp = src + ((size_t)gy * (size_t)W + (size_t)gx) * 3;
                        const float r = cp[0], g = cp[1], b = cp[2];
                        float m = r;
                        if (g > m) m = g;
                        if (b > m) m = b;
                        const float kk = m - A.threshold;
                        if (kk > 0.0f) {        // (a NaN m fails)
                            const float q = kk / m;
                            b0 = r * q; b1 = g * q; b2 = b * q;
                        }
                    }
                    const int at = sy * pitch + sx;
                    s0[at] = b0; s1[at] = b1; s2[at] = b2;
                    some = some || bloom_lit(b0) || bloom_lit(b1) || bloom_lit(b2);
                }
            }
            lit |= wave_any(some) ? 1u << k : 0u;
        }
        __syncthreads();
        // ---- the row taps of the tile's pixels, 32 x 8 at a time
#pragma unroll 1
        for (int k = 0; k < kTile / kTileRows; ++k) {
            const int row = ly + k * kTileRows;
            const int x = x0 + lx, y = ty0 + row;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            if ((lit >> k) & 1u)                // a scalar branch: this pair of rows has something bright in reach
                bloom_walk(s0, s1, s2, row * pitch + lx, 1, A, a0, a1, a2);
            if (x < W && y < y1) {
                float *op = hb + ((size_t)y * (size_t)W + (size_t)x) * 3;
                op[0] = a0; op[1] = a1; op[2] = a2;
            }
        }
        __syncthreads();                        // the next tile's staging overwrites what the taps read
    }
}

// crender_present_u8's cast (model_ops.hip): cvttss2si, then the low byte
__device__ inline unsigned char bloom_u8(float v)
{
    int iv = (int)0x80000000;
    if (v > -2147483904.0f && v < 2147483648.0f) iv = (int)v;
    return (unsigned char)((unsigned)iv & 0xFFu);
}

// Rules 5 and 6 on one channel.
__device__ inline float bloom_tone(float v, const BloomParams &A)
{
    float o = v;
    if (A.tone) {
        float a = v * A.exposure;
        a = a > 0.0f ? a : 0.0f;
        a = a * A.inv255;
        float L = a;
        if (A.reinhard) L = (a * (1.0f + a * A.iw2)) / (1.0f + a);
        if (A.gamma2) L = sqrtf(L);
        o = L * 255.0f;
    }
    return o > A.clamp ? A.clamp : o;           // (a NaN stays; a clamp of +inf is none)
}

template <bool U8>
__global__ __launch_bounds__(kThreads) void k_bloom_finish(const float *__restrict__ src, const float *__restrict__ hb,
                                                            BloomParams A, void *__restrict__ out, int W, int y0, int y1,
                                                            int tiles_x, int ntiles)
{
    extern __shared__ float s_bloom[];          // hb's r, g, b: [kTile + 2R][kTile] each; then a word per wavefront
    const int R = A.R, rows = kTile + 2 * R, plane = rows * kTile;
    float *const s0 = s_bloom, *const s1 = s_bloom + plane, *const s2 = s_bloom + 2 * plane;
    int *const s_lit = reinterpret_cast<int *>(s_bloom + 3 * plane);
    const auto [lane, wave, lx, ly] = tile_lane();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [x0, ty0] = tile_origin(tile, tiles_x, y0);
        // ---- stage hb of the tile and the R rows above and below it: a wavefront two rows at a time
        bool some = false;
        const int gx = x0 + lx;
        for (int sy = ly; sy < rows; sy += kTileRows) {
            const int gy = ty0 - R + sy;
            float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
            if (gy >= y0 && gy < y1 && gx < W) {
                const float *hp = hb + ((size_t)gy * (size_t)W + (size_t)gx) * 3;
                h0 = hp[0]; h1 = hp[1]; h2 = hp[2];
            }
            const int at = sy * kTile + lx;
            s0[at] = h0; s1[at] = h1; s2[at] = h2;
            some = some || bloom_lit(h0) || bloom_lit(h1) || bloom_lit(h2);
        }
        some = wave_any(some);
        if (lane == 0) s_lit[wave] = some ? 1 : 0;
        __syncthreads();
        int all = s_lit[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) all |= s_lit[w];
        const bool lit = wave_any(all != 0);    // a scalar branch: a dark tile walks nothing
        // ---- the column taps of the tile's pixels, 32 x 8 at a time; then rules 4 to 7
#pragma unroll 1
        for (int k = 0; k < kTile / kTileRows; ++k) {
            const int row = ly + k * kTileRows;
            const int x = x0 + lx, y = ty0 + row;
            float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
            if (lit) bloom_walk(s0, s1, s2, row * kTile + lx, kTile, A, g0, g1, g2);
            if (!(x < W && y < y1)) continue;
            const size_t pix = (size_t)y * (size_t)W + (size_t)x;
            const float *cp = src + pix * 3;
            float v0 = cp[0], v1 = cp[1], v2 = cp[2];
            const float t0 = A.intensity * g0, t1 = A.intensity * g1, t2 = A.intensity * g2;
            if (bloom_lit(t0) || bloom_lit(t1) || bloom_lit(t2)) {
                v0 = v0 + t0; v1 = v1 + t1; v2 = v2 + t2;
            }                                   // (otherwise the source's bits, a -0 and every NaN kept)
            v0 = bloom_tone(v0, A); v1 = bloom_tone(v1, A); v2 = bloom_tone(v2, A);
            const size_t opix = (size_t)(A.flip ? A.H - 1 - y : y) * (size_t)W + (size_t)x;
            if constexpr (U8) {
                unsigned char *op = reinterpret_cast<unsigned char *>(out) + opix * 3;
                op[0] = bloom_u8(v0); op[1] = bloom_u8(v1); op[2] = bloom_u8(v2);
            } else {
                float *op = reinterpret_cast<float *>(out) + opix * 3;
                op[0] = v0; op[1] = v1; op[2] = v2;
            }
        }
        __syncthreads();                        // the next tile's staging overwrites what the taps read
    }
}

}  // namespace

extern "C" {

int crender_bloom(const float *d_src, float threshold, const float *weights, int radius, float intensity, float exposure,
                  float inv_white2, float clamp, float *d_scratch, void *d_out, int H, int W, int y0, int y1, unsigned flags,
                  void *stream)
{
    const char *const E = "crender_bloom";
    if (int rc = frame_checks(E, 0, true, H, W)) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (!d_src || !weights || !d_scratch || !d_out) return arg_error(E, "d_src, weights, d_scratch or d_out is NULL");
    if (radius < 1 || radius > CRENDER_BLOOM_MAX_RADIUS) return arg_error(E, "radius is not 1 .. 32");
    for (int k = 0; k <= radius; ++k)
        if (!isfinite(weights[k])) return arg_error(E, "a weight is not finite");
    if (!(threshold >= 0.0f)) return arg_error(E, "threshold is negative or NaN");
    if (!isfinite(intensity) || intensity < 0.0f) return arg_error(E, "intensity is not finite and 0 or above");
    if (!isfinite(exposure) || exposure < 0.0f) return arg_error(E, "exposure is not finite and 0 or above");
    if (!(inv_white2 >= 0.0f)) return arg_error(E, "inv_white2 is negative or NaN");
    if (clamp != clamp) return arg_error(E, "clamp is NaN");
    const unsigned known = CRENDER_BLOOM_U8 | CRENDER_BLOOM_FLIP | CRENDER_BLOOM_REINHARD | CRENDER_BLOOM_GAMMA2;
    if (flags & ~known) return arg_error(E, "unknown flag bits");
    if (d_out == (const void *)d_src || d_out == (const void *)d_scratch || d_scratch == d_src)
        return arg_error(E, "d_out, d_scratch and d_src are not three planes (the pass cannot run in place)");
    int tiles_x, tiles;
    if (int rc = tile_grid(E, W, y0, y1, tiles_x, tiles)) return rc;
    BloomParams A = {};
    A.threshold = threshold; A.intensity = intensity; A.exposure = exposure;
    A.inv255 = (float)(1.0 / 255.0); A.iw2 = inv_white2; A.clamp = clamp;
    A.R = radius; A.H = H;
    A.reinhard = (flags & CRENDER_BLOOM_REINHARD) ? 1 : 0;
    A.gamma2 = (flags & CRENDER_BLOOM_GAMMA2) ? 1 : 0;
    A.tone = (A.reinhard || A.gamma2 || exposure != 1.0f) ? 1 : 0;
    A.flip = (flags & CRENDER_BLOOM_FLIP) ? 1 : 0;
    for (int k = 0; k <= radius; ++k) A.w[k] = weights[k];
    const dim3 grid((unsigned)(tiles < kBloomMaxGrid ? tiles : kBloomMaxGrid));
    const size_t lds = (size_t)3 * kTile * (kTile + 2 * radius) * 4;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_bloom_rows, grid, dim3(kThreads), lds, st, d_src, A, d_scratch, W, y0, y1, tiles_x, tiles);
    CR_LAUNCH_CHECK("k_bloom_rows");
    if (flags & CRENDER_BLOOM_U8)
        hipLaunchKernelGGL(k_bloom_finish<true>, grid, dim3(kThreads), lds + (kThreads / 64) * 4, st, d_src,
                           (const float *)d_scratch, A, d_out, W, y0, y1, tiles_x, tiles);
    else
        hipLaunchKernelGGL(k_bloom_finish<false>, grid, dim3(kThreads), lds + (kThreads / 64) * 4, st, d_src,
                           (const float *)d_scratch, A, d_out, W, y0, y1, tiles_x, tiles);
    CR_LAUNCH_CHECK("k_bloom_finish");
    return CRENDER_OK;
}

}  // extern "C"

// ---- transparency (crender_peel_next, crender_peel_blend) ----
// Depth peeling by depth key.  A frame leaves the two halves of every pixel's winning key behind, the z plane and the
// winner plane; the layer behind it is, per pixel, the fragment with the LEAST key strictly above that one: no epsilon,
// coplanar duplicates peel one by one, and being a minimum of unique 64-bit keys it comes out bit for bit whatever the
// launch order.  crender_peel_next is crender_raster_atomic's walk (raster.hip: k_keys_init, k_cover_atomic,
// k_resolve_global) with one more test per sample, three launches:
//   k_peel_seed     a pixel per work item: the key plane gets the cleared key where the previous layer is valid (its
//                   winner is a triangle, its z is not NaN) and 0 where it is not — no key is below 0, so an exhausted
//                   pixel never takes a fragment and the cover pass needs no validity test of its own.
//   k_peel_cover    a wavefront per triangle of the caller's order (through pos_of to where it lies in d_tri), 8 x 8
//                   pixels per step over the pixel box clipped to the rows.  Per sample: the barycentrics (three correctly
//                   rounded divisions) and z, as every coverage pass pays them; for a sample that is a fragment 16 bytes
//                   of plain loads — the slot's key, then the previous winner and z, from which K is rebuilt — and the
//                   64-bit atomicMin only if K < k and k < *slot (the slot only ever falls, so a stale read costs an
//                   atomic, never a result).  A wavefront owns its triangle's WHOLE box: one frame-sized triangle is
//                   (W / 8) (H / 8) serial steps of one wavefront (1 024 at 256^2, 262 144 at 4096^2) while the rest of
//                   the device idles; boxes are not split among wavefronts.  The grid is capped at kPeelMaxGrid
//                   workgroups, 4 wavefronts each: beyond 32 768 triangles a wavefront takes further trips.
//   k_peel_resolve  a pixel per work item: the slot's low word names the fragment, whose z is computed again by the same
//                   device functions — the very value the key was built from, a -0 as -0 — and stored with the index;
//                   a slot still at its seed stores winner -1 and z 1e6f.
// crender_peel_blend puts one layer under what is in front of it, a per-pixel pass of the shape of k_env_shade: a pixel
// per lane, no LDS, 4 bytes of winner a pixel and for a pixel that blends its transmittance, alpha, the winner's 27
// floats of corners, colours and normals (or 12 bytes of the front plane), three divisions, and 16 bytes stored.

namespace {

constexpr int kPeelMaxGrid = 8192;           // workgroups of the cover launch: 32 768 wavefronts; the kernel loops

// Whether the previous layer's pixel names a fragment, and then its key.
__device__ inline bool peel_prev_key(int32_t w, float z, int64_t T, const uint32_t *__restrict__ pos_of,
                                     unsigned long long &K)
{
    if (w < 0 || (int64_t)w >= T || z != z) return false;
    if (pos_of && (int64_t)pos_of[w] >= T) return false;
    K = fragment_key(z, (uint32_t)w);
    return true;
}

__global__ __launch_bounds__(kThreads) void k_peel_seed(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                         int64_t T, const uint32_t *__restrict__ pos_of,
                                                         unsigned long long *__restrict__ keys, size_t first_pix,
                                                         size_t npix)
{
    const size_t stride = (size_t)gridDim.x * kThreads;
    const unsigned long long key_clear = make_key(zord(1e6f), KEY_LOW_PRIOR);
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += stride) {
        const size_t pix = first_pix + i;
        unsigned long long K;
        keys[pix] = peel_prev_key(win[pix], zb[pix], T, pos_of, K) ? key_clear : 0ull;
    }
}

__global__ __launch_bounds__(kThreads) void k_peel_cover(const int32_t *__restrict__ win, const float *__restrict__ zb,
                                                          const float *__restrict__ tri, const float *__restrict__ nrm,
                                                          int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                          unsigned long long *__restrict__ keys, int W, int H, int y0,
                                                          int y1)
{
    const int l = threadIdx.x & 63, lx = l & 7, ly = l >> 3;
    const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * kThreads) >> 6;
    for (int64_t i = wave; i < T; i += nwaves) {             // i: the caller's index, the winner plane's word
        const int64_t t = pos_of ? (int64_t)pos_of[i] : i;
        if (t >= T) continue;
        const float *nn = nrm + t * 9;
        if (backface(nn[2], nn[5], nn[8])) continue;
        const TriXYZ tr = winner_triangle(tri, t, P);
        int xl, xr, yt, yb;
        pixel_box(tr.x0, tr.y0, tr.x1, tr.y1, tr.x2, tr.y2, W, H, xl, xr, yt, yb);
        if (xl - xr == 0 || yt - yb == 0) continue;
        if (yt < y0) yt = y0;
        if (yb > y1) yb = y1;
        for (int yy = yt + ly; yy < yb; yy += 8)
            for (int xx = xl + lx; xx < xr; xx += 8) {
                unsigned long long k;
                if (!fragment(tr, (uint32_t)i, xx, yy, k)) continue;
                const size_t pix = (size_t)yy * (size_t)W + (size_t)xx;
                unsigned long long *slot = &keys[pix];
                if (!(k < *slot)) continue;                  // (0 where the previous layer is not valid)
                const unsigned long long K = fragment_key(zb[pix], (uint32_t)win[pix]);
                if (K < k) atomicMin(slot, k);
            }
    }
}

__global__ __launch_bounds__(kThreads) void k_peel_resolve(const float *__restrict__ tri,
                                                            const uint32_t *__restrict__ pos_of, ProjConst P,
                                                            const unsigned long long *__restrict__ keys,
                                                            int32_t *__restrict__ win_out, float *__restrict__ z_out, int W,
                                                            size_t first_pix, size_t npix)
{
    const size_t stride = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < npix; i += stride) {
        const size_t pix = first_pix + i;
        const unsigned long long key = keys[pix];
        const uint32_t low = (uint32_t)key;
        int32_t w = -1;
        float z = 1e6f;
        if (key != 0ull && low != KEY_LOW_PRIOR) {
            const uint32_t id = 0xFFFFFFFEu - low;
            const int64_t t = pos_of ? (int64_t)pos_of[id] : (int64_t)id;
            const TriXYZ tr = winner_triangle(tri, t, P);
            float b1, b2, b3;
            barycentric(tr, (int)(pix % (size_t)W), (int)(pix / (size_t)W), b1, b2, b3);
            z = interp(tr.z0, tr.z1, tr.z2, b1, b2, b3);
            w = (int32_t)id;
        }
        win_out[pix] = w;
        z_out[pix] = z;
    }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kThreads) void k_peel_blend(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                          int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                          const float *__restrict__ col, const float *__restrict__ nrm,
                                                          const float *__restrict__ alpha, Light L,
                                                          const float *__restrict__ front, float bg0, float bg1, float bg2,
                                                          float *__restrict__ trans, float *__restrict__ ob, int W, int y0,
                                                          int y1, int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!FIRST && !LAST && !wave_any(px.covered)) continue;     // a scalar branch: the whole wavefront leaves
        if (!px.inside) continue;
        float *op = ob + px.pix * 3;
        float t = FIRST ? 1.0f : trans[px.pix];
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
        bool wrote = false;
        if (px.covered && t > 0.0f) {
            float a = alpha[px.orig];
            a = a > 0.0f ? a : 0.0f;                                 // (a NaN gives 0)
            a = a > 1.0f ? 1.0f : a;
            float c0, c1, c2;
            if (FIRST && front) {
                const float *fp = front + px.pix * 3;
                c0 = fp[0]; c1 = fp[1]; c2 = fp[2];
            } else {
                const TriXYZ X = winner_triangle(tri, px.t, P);
                float c[9], n[9], b1, b2, b3;
                load9(col + px.t * 9, c);
                load9(nrm + px.t * 9, n);
                barycentric(X, px.x, px.y, b1, b2, b3);
                const Shade s = shade_fragment(c, n, b1, b2, b3, L);
                c0 = s.c0; c1 = s.c1; c2 = s.c2;
            }
            const float g = t * a;
            if (FIRST) {
                o0 = g * c0; o1 = g * c1; o2 = g * c2;
            } else {
                o0 = op[0] + g * c0; o1 = op[1] + g * c1; o2 = op[2] + g * c2;
            }
            t = t * (1.0f - a);
            wrote = true;
        } else if (FIRST) {
            wrote = true;                                            // no triangle: out = 0, trans = 1
        }
        if (LAST && t > 0.0f) {
            if (!wrote) { o0 = op[0]; o1 = op[1]; o2 = op[2]; }
            o0 = o0 + t * bg0; o1 = o1 + t * bg1; o2 = o2 + t * bg2;
            op[0] = o0; op[1] = o1; op[2] = o2;
            if (wrote) trans[px.pix] = t;
        } else if (wrote) {
            op[0] = o0; op[1] = o1; op[2] = o2;
            trans[px.pix] = t;
        }
    }
}

}  // namespace

extern "C" {

int crender_peel_next(const int32_t *d_winner, const float *d_z, const float *d_tri, int64_t T, const uint32_t *d_pos_of,
                      const float *P16, const float *d_nrm, void *d_keys, int32_t *d_winner_out, float *d_z_out, int H,
                      int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_peel_next";
    if (!d_winner || !d_z || !P16 || !d_keys || !d_winner_out || !d_z_out)
        return arg_error(E, "d_winner, d_z, P16, d_keys, d_winner_out or d_z_out is NULL");
    if (int rc = frame_checks(E, T, d_tri && d_nrm, H, W, "d_tri or d_nrm is NULL with T > 0")) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags) return arg_error(E, "unknown flag bits");
    if (T > 0x7FFFFFFFll) return arg_error(E, "T is above 2^31 - 1 (the winner plane is int32)");
    if (d_winner_out == d_winner || d_z_out == d_z) return arg_error(E, "an output plane is its input (the peel cannot run in place)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t first = (size_t)y0 * (size_t)W, npix = (size_t)(y1 - y0) * (size_t)W;
    unsigned long long *keys = static_cast<unsigned long long *>(d_keys);
    const ProjConst P = make_proj(P16, W, H);
    hipLaunchKernelGGL(k_peel_seed, dim3(grid_for(npix, 4096)), dim3(kThreads), 0, s, d_winner, d_z, T, d_pos_of, keys, first,
                       npix);
    CR_LAUNCH_CHECK("k_peel_seed");
    if (T > 0) {
        hipLaunchKernelGGL(k_peel_cover, dim3(grid_for((size_t)T * 64, kPeelMaxGrid)), dim3(kThreads), 0, s, d_winner, d_z,
                           d_tri, d_nrm, T, d_pos_of, P, keys, W, H, y0, y1);
        CR_LAUNCH_CHECK("k_peel_cover");
    }
    hipLaunchKernelGGL(k_peel_resolve, dim3(grid_for(npix, 8192)), dim3(kThreads), 0, s, d_tri, d_pos_of, P, keys,
                       d_winner_out, d_z_out, W, first, npix);
    CR_LAUNCH_CHECK("k_peel_resolve");
    return CRENDER_OK;
}

int crender_peel_blend(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of, const float *P16,
                       const float *d_col, const float *d_nrm, const float *d_alpha, const float *light3,
                       const float *d_front, const float *background3, float *d_trans, float *d_out, int H, int W, int y0,
                       int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_peel_blend";
    const bool first = flags & CRENDER_PEEL_FIRST, last = flags & CRENDER_PEEL_LAST;
    if (!d_winner || !P16 || !background3 || !d_trans || !d_out)
        return arg_error(E, "d_winner, P16, background3, d_trans or d_out is NULL");
    if (int rc = frame_checks(E, T, d_tri && d_col && d_nrm && d_alpha, H, W, "d_tri, d_col, d_nrm or d_alpha is NULL with T > 0"))
        return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (flags & ~(unsigned)(CRENDER_PEEL_FIRST | CRENDER_PEEL_LAST)) return arg_error(E, "unknown flag bits");
    if (d_front && !first) return arg_error(E, "d_front is given without CRENDER_PEEL_FIRST");
    if (d_front == d_out) return arg_error(E, "d_out is d_front (the blend cannot run in place)");
    if (!(isfinite(background3[0]) && isfinite(background3[1]) && isfinite(background3[2])))
        return arg_error(E, "background3 is not finite");
    if (light3 && !(isfinite(light3[0]) && isfinite(light3[1]) && isfinite(light3[2])))
        return arg_error(E, "light3 is not finite");
    const ProjConst P = make_proj(P16, W, H);
    static constexpr decltype(&k_peel_blend<false, false>) kernels[2][2] = {
        {k_peel_blend<false, false>, k_peel_blend<false, true>}, {k_peel_blend<true, false>, k_peel_blend<true, true>}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[first][last], G.grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner, d_tri, T,
                       d_pos_of, P, d_col, d_nrm, d_alpha, pass_light(light3), d_front, background3[0], background3[1],
                       background3[2], d_trans, d_out, W, y0, y1, G.row_blocks);
    CR_LAUNCH_CHECK("k_peel_blend");
    return CRENDER_OK;
}

}  // extern "C"

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
    for (int i : {1, 2, 4, 6, 8, 9, 12, 13})
        if (!(P16[i] == 0.0f))
            return arg_error(E, "P16 is not of crender_projection_matrix's shape (an entry that must be 0 is not)");
    for (int i : {0, 5, 14})
        if (!isfinite(P16[i]) || P16[i] == 0.0f)
            return arg_error(E, "P16 is not of crender_projection_matrix's shape (entry 0, 5 or 14 is 0 or not finite)");
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

// ---- normal mapping (crender_nmap_from_height, crender_nmap_shade) ------------------------------------------------
// A deferred pass that rewrites the NORMAL plane for the covered pixels, once and right after the draw: every pass that
// lights a pixel reads that plane (the illumination pass, the fused light of the texture passes and of the resolve,
// k_phong_shade, k_ao_shade), so all of them get the bumps without a change.  The shape of k_tex_shade (texture.hip): a
// pixel per work item, an 8 x 8 block of pixels per wavefront, a grid-stride loop over row blocks; a wavefront whose 64
// winners are all background leaves after its one load.  A covered pixel projects its winner, takes (u, v) from the
// rasterizer's barycentrics (for the trilinear filter also at its right and lower neighbour: two more barycentric
// triples of the same triangle, whose nine edge constants the compiler keeps), samples the map, builds the tangent frame
// of the triangle from its unprojected corners and its uv, turns it around the stored normal and stores the sum.  What
// the pass needs of the mip unit — the chain's layout and the level of a footprint, crender_mip.h's statements — is
// restated here: that unit's headers are its own.  The level offsets travel by value in the kernel's arguments.

namespace {

constexpr int kNmapMaxLevels = 16;           // a side is at most 65 535
enum { kNmapNearest = 0, kNmapBilinear = 1, kNmapTrilinear = 2 };

// The map of a call: its size and, for a chain, where each level starts (crender_mip_build's layout).
struct NmapChain {
    unsigned long long off[kNmapMaxLevels];
    int mh, mw, L;
};

NmapChain nmap_chain(int mh, int mw, bool chain)
{
    NmapChain M{};
    M.mh = mh;
    M.mw = mw;
    M.L = 1;
    if (chain) {
        const int side = mh > mw ? mh : mw;
        M.L = 0;
        while ((side >> M.L) > 0) ++M.L;     // 1 + floor(log2(side))
        unsigned long long total = 0;
        for (int k = 0; k < M.L; ++k) {
            const int h = (mh >> k) > 1 ? (mh >> k) : 1, w = (mw >> k) > 1 ? (mw >> k) : 1;
            M.off[k] = total;
            total += 3ull * (unsigned long long)h * (unsigned long long)w;
        }
    }
    return M;
}

// The Level statement of crender_mip.h: the lower level l0 and the weight f of the one above it.
CR_DEV void nmap_level(float rho, int L, int &l0, float &f)
{
    l0 = 0;
    f = 0.0f;
    if (rho > 1.0f) {
        if (!(rho < (float)(1u << (L - 1)))) {
            l0 = L - 1;
        } else {
            // 1 < rho < 2^15: the exponent field is the level, the significand scaled back by the exact power is 1 + f
            l0 = (int)(__float_as_uint(rho) >> 23) - 127;
            f = rho * __uint_as_float((uint32_t)(127 - l0) << 23) - 1.0f;
        }
    }
}

// (u, v) of the integer pixel (x, y) in projected triangle X: the Affine or the Perspective statement of crender_tex.h.
template <bool PERSPECTIVE>
CR_DEV void nmap_uv(const TriXYZ &X, float za, float zb, float zc, const float w[6], int x, int y, float &tu, float &tv)
{
    float b1, b2, b3;
    barycentric(X, x, y, b1, b2, b3);
    if (PERSPECTIVE) {
        const float q1 = b1 / za, q2 = b2 / zb, q3 = b3 / zc;
        const float s = (q1 + q2) + q3;
        tu = ((w[0] * q1 + w[2] * q2) + w[4] * q3) / s;
        tv = ((w[1] * q1 + w[3] * q2) + w[5] * q3) / s;
    } else {
        tu = interp(w[0], w[2], w[4], b1, b2, b3);
        tv = interp(w[1], w[3], w[5], b1, b2, b3);
    }
}

CR_DEV float nmap_dot(const float a[3], const float b[3])
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

template <bool PERSPECTIVE, int FILTER>
__global__ __launch_bounds__(kThreads) void k_nmap_shade(const int32_t *__restrict__ win, const float *__restrict__ tri,
                                                          int64_t T, const uint32_t *__restrict__ pos_of, ProjConst P,
                                                          const float *__restrict__ uv,
                                                          const unsigned char *__restrict__ map, NmapChain M,
                                                          float strength, float *__restrict__ nb, int W, int y0, int y1,
                                                          int row_blocks)
{
    for (int rb = blockIdx.y; rb < row_blocks; rb += gridDim.y) {
        const WinnerPixel px = winner_pixel(win, T, pos_of, W, y0, y1, rb);
        if (!wave_any(px.covered)) continue;        // a scalar branch: the whole wavefront leaves
        if (!px.covered) continue;
        float raw[3][3];
        const TriXYZ X = winner_triangle(tri, px.t, P, raw);
        const float *wp = uv + px.orig * 6;
        const float w[6] = {wp[0], wp[1], wp[2], wp[3], wp[4], wp[5]};
        // ---- 1, 2: the sample
        float tu, tv, s[3];
        nmap_uv<PERSPECTIVE>(X, raw[0][2], raw[1][2], raw[2][2], w, px.x, px.y, tu, tv);
        if (FILTER == kNmapTrilinear) {
            float ux, vx, uy, vy;
            nmap_uv<PERSPECTIVE>(X, raw[0][2], raw[1][2], raw[2][2], w, px.x + 1, px.y, ux, vx);
            nmap_uv<PERSPECTIVE>(X, raw[0][2], raw[1][2], raw[2][2], w, px.x, px.y + 1, uy, vy);
            const float fmw = (float)M.mw, fmh = (float)M.mh;
            const float dudx = (ux - tu) * fmw, dvdx = (vx - tv) * fmh;
            const float dudy = (uy - tu) * fmw, dvdy = (vy - tv) * fmh;
            const float rx = dudx * dudx + dvdx * dvdx;
            const float ry = dudy * dudy + dvdy * dvdy;
            const float r2 = (rx >= ry) ? rx : ry;
            const float rho = sqrtf(r2);
            int l0;
            float f;
            nmap_level(rho, M.L, l0, f);
            const int hl = max(1, M.mh >> l0), wl = max(1, M.mw >> l0);
            bilinear(map + (l0 ? M.off[l0] : 0ull), hl, wl, tu, tv, s);
            if (f != 0.0f) {         // (only between two levels: l0 + 1 <= L - 1)
                float up[3];
                bilinear(map + M.off[l0 + 1], max(1, hl >> 1), max(1, wl >> 1), tu, tv, up);
                const float g = 1.0f - f;
#pragma unroll
                for (int j = 0; j < 3; ++j) s[j] = s[j] * g + up[j] * f;
            }
        } else if (FILTER == kNmapBilinear) {
            bilinear(map, M.mh, M.mw, tu, tv, s);
        } else {
            const int row = clipi(host_f32_to_i32((1.0f - tv) * (float)M.mh), 0, M.mh - 1);
            const int colm = clipi(host_f32_to_i32(tu * (float)M.mw), 0, M.mw - 1);
            const unsigned char *p = texel(map, row, colm, M.mw);
            s[0] = (float)p[0]; s[1] = (float)p[1]; s[2] = (float)p[2];
        }
        float m[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            m[j] = (s[j] - 128.0f) / 127.0f;
            m[j] = m[j] < -1.0f ? -1.0f : m[j];
        }
        const float mx = m[0] * strength, my = m[1] * strength, mz = m[2];
        // ---- 3: the tangent frame of the triangle
        const float du1 = w[2] - w[0], dv1 = w[3] - w[1], du2 = w[4] - w[0], dv2 = w[5] - w[1];
        const float det = du1 * dv2 - du2 * dv1;
        const float sg = det < 0.0f ? -1.0f : 1.0f;
        float Tt[3], Bt[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float e1 = raw[1][j] - raw[0][j], e2 = raw[2][j] - raw[0][j];
            Tt[j] = (e1 * dv2 - e2 * dv1) * sg;
            Bt[j] = (e2 * du1 - e1 * du2) * sg;
        }
        // ---- 4: the frame around the stored normal
        float *np_ = nb + px.pix * 3;
        const float n[3] = {np_[0], np_[1], np_[2]};
        const float nl = sqrtf(nmap_dot(n, n));
        const float Nu[3] = {n[0] / nl, n[1] / nl, n[2] / nl};
        const float d = nmap_dot(Nu, Tt);
        const float Tp[3] = {Tt[0] - Nu[0] * d, Tt[1] - Nu[1] * d, Tt[2] - Nu[2] * d};
        const float tl = sqrtf(nmap_dot(Tp, Tp));
        const float Tu[3] = {Tp[0] / tl, Tp[1] / tl, Tp[2] / tl};
        float Bp[3] = {Nu[1] * Tu[2] - Nu[2] * Tu[1], Nu[2] * Tu[0] - Nu[0] * Tu[2], Nu[0] * Tu[1] - Nu[1] * Tu[0]};
        if (nmap_dot(Bp, Bt) < 0.0f) {
            Bp[0] = -Bp[0]; Bp[1] = -Bp[1]; Bp[2] = -Bp[2];
        }
        // ---- 5, 6: the result, where there is a frame and something to tilt by (false for every NaN)
        const bool tilt = mx < 0.0f || mx > 0.0f || my < 0.0f || my > 0.0f;
        if ((det > 0.0f || det < 0.0f) && nl > 0.0f && tl > 0.0f && tilt) {
#pragma unroll
            for (int j = 0; j < 3; ++j) np_[j] = (Tu[j] * mx + Bp[j] * my) + Nu[j] * mz;
        }
    }
}

// A texel per work item in a grid-stride loop: the statements of crender_nmap_from_height.
__global__ __launch_bounds__(kThreads) void k_nmap_from_height(const uint8_t *__restrict__ hm, int mh, int mw, float k,
                                                                int wrap, uint8_t *__restrict__ out)
{
    const size_t n = (size_t)mh * (size_t)mw;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const int r = (int)(i / (size_t)mw), c = (int)(i - (size_t)r * (size_t)mw);
        int cl = c - 1, cr = c + 1, ru = r - 1, rd = r + 1;
        if (wrap) {
            cl = cl < 0 ? mw - 1 : cl;
            cr = cr >= mw ? 0 : cr;
            ru = ru < 0 ? mh - 1 : ru;
            rd = rd >= mh ? 0 : rd;
        } else {
            cl = cl < 0 ? 0 : cl;
            cr = cr >= mw ? mw - 1 : cr;
            ru = ru < 0 ? 0 : ru;
            rd = rd >= mh ? mh - 1 : rd;
        }
        const uint8_t *row = hm + (size_t)r * (size_t)mw;
        const float gx = (float)((int)row[cr] - (int)row[cl]) * k;
        const float gy = (float)((int)hm[(size_t)ru * (size_t)mw + (size_t)c] - (int)hm[(size_t)rd * (size_t)mw + (size_t)c]) * k;
        const float ln = sqrtf((gx * gx + gy * gy) + 1.0f);
        const float v[3] = {-gx / ln, -gy / ln, 1.0f / ln};
        uint8_t *o = out + i * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float b = rintf(v[j] * 127.0f + 128.0f);
            o[j] = (uint8_t)(int)(!(b > 0.0f) ? 0.0f : (b > 255.0f ? 255.0f : b));      // (a NaN gives 0)
        }
    }
}

}  // namespace

extern "C" {

int crender_nmap_from_height(const uint8_t *d_height, int mh, int mw, float scale, unsigned flags, uint8_t *d_map,
                             void *stream)
{
    const char *const E = "crender_nmap_from_height";
    if (!d_height || !d_map) return arg_error(E, "d_height or d_map is NULL");
    if (mh < 1 || mw < 1 || mh > 65535 || mw > 65535) return arg_error(E, "mh or mw is not 1 .. 65535");
    if (!isfinite(scale)) return arg_error(E, "scale is not finite");
    if (flags & ~(unsigned)CRENDER_NMAP_WRAP) return arg_error(E, "unknown flag bits");
    const float k = scale / 255.0f;
    hipLaunchKernelGGL(k_nmap_from_height, dim3(grid_for((size_t)mh * (size_t)mw, 16384)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), d_height, mh, mw, k, (flags & CRENDER_NMAP_WRAP) ? 1 : 0, d_map);
    CR_LAUNCH_CHECK("k_nmap_from_height");
    return CRENDER_OK;
}

int crender_nmap_shade(const int32_t *d_winner, const float *d_tri, int64_t T, const uint32_t *d_pos_of, const float *P16,
                       const float *d_uv, const uint8_t *d_map, int mh, int mw, float strength, float *d_normal, int H,
                       int W, int y0, int y1, unsigned flags, void *stream)
{
    const char *const E = "crender_nmap_shade";
    if (!d_winner || !P16 || !d_map || !d_normal) return arg_error(E, "d_winner, P16, d_map or d_normal is NULL");
    if (int rc = frame_checks(E, T, d_tri && d_uv, H, W, "d_tri or d_uv is NULL with T > 0")) return rc;
    if (int rc = rows_check(E, H, y0, y1)) return rc;
    if (mh < 1 || mw < 1 || mh > 65535 || mw > 65535) return arg_error(E, "mh or mw is not 1 .. 65535");
    if (!isfinite(strength)) return arg_error(E, "strength is not finite");
    const bool persp = flags & CRENDER_NMAP_PERSPECTIVE, bilin = flags & CRENDER_NMAP_BILINEAR, chain = flags & CRENDER_NMAP_CHAIN;
    if (flags & ~(unsigned)(CRENDER_NMAP_PERSPECTIVE | CRENDER_NMAP_BILINEAR | CRENDER_NMAP_CHAIN))
        return arg_error(E, "unknown flag bits");
    if (chain && bilin) return arg_error(E, "CRENDER_NMAP_CHAIN with CRENDER_NMAP_BILINEAR");
    if (T == 0) return CRENDER_OK;
    // [perspective][filter]
    static constexpr decltype(&k_nmap_shade<false, kNmapNearest>) kernels[2][3] = {
        {k_nmap_shade<false, kNmapNearest>, k_nmap_shade<false, kNmapBilinear>, k_nmap_shade<false, kNmapTrilinear>},
        {k_nmap_shade<true, kNmapNearest>, k_nmap_shade<true, kNmapBilinear>, k_nmap_shade<true, kNmapTrilinear>}};
    const PassGrid G = pass_grid(W, y0, y1);
    hipLaunchKernelGGL(kernels[persp][chain ? kNmapTrilinear : (bilin ? kNmapBilinear : kNmapNearest)], G.grid,
                       dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_winner, d_tri, T, d_pos_of,
                       make_proj(P16, W, H), d_uv, d_map, nmap_chain(mh, mw, chain), strength, d_normal, W, y0, y1,
                       G.row_blocks);
    CR_LAUNCH_CHECK("k_nmap_shade");
    return CRENDER_OK;
}

}  // extern "C"

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
