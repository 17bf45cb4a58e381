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
