// frame32.hip — the swap chain's frame kernel for small scenes on 32-pixel tiles (include/crender_frame32.h).
//
// One launch per frame, like k_frame (raster.hip): [nsetup binning wavefronts of the slot's NEXT frame]
// [3 * hmax helper workgroups][ntiles main workgroups, raster order with the 9 * ty row rotation].  Nothing in
// the launch waits for anything else in it.  What differs from k_frame<32, true> is what is NOT here: the frames
// that qualify (frame32_raster_pass) have direct bins, a fused clear, no winner plane, no light, no triangle order and
// 32-bit offsets, and the class statistics say their records are small — so a covered tile is queued in batches of
// 256 records and every batch is swept run-wise (the shape of raster.hip's sweep_runs32, exact for records of any
// size), then resolved.  No block sweep, no pixel owners, no dispatch order, no pair lists, no hash resolve.
//
// All sample arithmetic is raster_math.h's (make_setup, numerators, fragment_from, quotients, store_fragment,
// shade_and_store, the depth keys), the binning wavefronts are binning.h's setup_wave_body<32, true>: the planes are
// the general kernel's bit for bit.  The plans are shared with the general kernels, so the cross-frame protocol is
// kept word for word (see raster.hip, pick_tile / raster_body):
//   count_next[tile] = 0            by each tile's own workgroup
//   heavy_flag / heavy_slots        read by the parts of a split tile, zeroed once every wavefront has read them
//   heavy_ctr_next, hint_bad_next   zeroed by main workgroup 0
//   stats_prev, the usage record    summed, zeroed and written by the last main workgroup: two 16-byte stores, the
//                                   sequence word leading the first and trailing the second
//   the tile's size class           one atomic, the tile's last memory operation
//   a list                          clamps to `capacity`; entries with a triangle index >= T are ignored
//
// Slotted keys.  Direct bins mean T <= 65536, so a depth key's low word has room for more than the index: its high
// half is 0xFFFF - index (the compared bits: the tie rule is untouched), its low half the batch (8 bits) and the
// record's slot in the queue (8 bits), as on 16-pixel tiles.  A pixel whose winner came with the list's LAST batch —
// every winner of a list of up to 256 records — takes coordinates, denominators and refined reciprocals from the
// queue in LDS: no gather of the projected vertices and no division set-up per pixel.  Other winners go through
// shade_and_store from global memory.
//
// Row stores.  Where the frame's rows are 16-byte aligned (the clear's condition, A.vec_clear) a covered rectangle of
// full width leaves its wavefronts as whole rows in 16-byte write-through stores, like an empty tile's
// (resolve_tile_rows); a rectangle cut at the frame's right edge, and every rectangle of any other frame, is stored
// pixel by pixel (resolve_tile).  Same words either way.
#include <mutex>
#include <unordered_map>

#include "plan.h"
#include "../../include/crender_frame32.h"

using namespace crender_detail;

namespace {

constexpr int TS = 32;
#ifdef CRENDER_FRAME32_PLAIN_KEYS          // (A/B build: the general kernel's keys, every winner from global memory)
constexpr bool kSlotted = false;
#else
constexpr bool kSlotted = true;
#endif
#ifdef CRENDER_FRAME32_PLAIN_STORES        // (A/B build: every covered tile resolved by per-pixel plain stores)
constexpr bool kRowStores = false;
#else
constexpr bool kRowStores = true;
#endif

// slot of tile-local pixel (dx, dy) in the key plane: each row's pairs of keys permuted by the row number
// (raster.hip, key_slot<32>)
CR_DEV int key_slot(int dx, int dy) { return dy * 32 + (dx ^ ((dy << 1) & 30)); }

// One batch of a tile's list, slot = thread index: the record's coordinates, what depends on the triangle alone and
// is more than one operation away (denominators, refined reciprocals; r1 = 0: outside the division window), the
// word fragment_from turns into the key's low word, the clipped box and the prefix of the item counts.
struct Queue {
    float x0[kThreads], y0[kThreads], z0[kThreads];
    float x1[kThreads], y1[kThreads], z1[kThreads];
    float x2[kThreads], y2[kThreads], z2[kThreads];
    float l03[kThreads], l13[kThreads], l23[kThreads];
    float r1[kThreads], r2[kThreads], r3[kThreads];
    uint32_t tri[kThreads];      // 0xFFFFFFFE - (low word of the record's keys): fragment_key's `tri`
    // tile-local clipped box: x0 | y0 << 6 | w << 12 | h << 19 (w = 0: no work); bits 26..31: how many records
    // WITHOUT work follow this one in its wavefront's 64 slots
    uint32_t box[kThreads];
    uint32_t px_scan[kThreads];  // exclusive prefix of the records' item counts within the wavefront
    uint32_t wave_px[kThreads / 64];
};
static_assert(kSetupWaveLds <= sizeof(Queue), "a binning wavefront works in the batch queue");

CR_DEV uint32_t pack_box(uint32_t xy, uint32_t wh, int X0, int Y0)
{
    if (wh == 0) return 0u;
    return (uint32_t)((int)(xy & 0xFFFF) - X0) | ((uint32_t)((int)(xy >> 16) - Y0) << 6) | ((wh & 0x7Fu) << 12) |
           ((wh >> 16) << 19);
}
CR_DEV int packed_w(uint32_t b) { return (int)((b >> 12) & 0x7Fu); }
CR_DEV int packed_h(uint32_t b) { return (int)((b >> 19) & 0x7Fu); }
CR_DEV uint32_t packed_skip(uint32_t b) { return b >> 26; }

CR_DEV TriSetup queued_setup(const Queue &q, int r)
{
    TriSetup st;
    st.x0 = q.x0[r]; st.y0 = q.y0[r]; st.z0 = q.z0[r];
    st.x1 = q.x1[r]; st.y1 = q.y1[r]; st.z1 = q.z1[r];
    st.x2 = q.x2[r]; st.y2 = q.y2[r]; st.z2 = q.z2[r];
    st.l01 = st.x1 - st.x2; st.l02 = st.y1 - st.y2;      // (make_setup's own operations, one each)
    st.l11 = st.x2 - st.x0; st.l12 = st.y2 - st.y0;
    st.l21 = st.x0 - st.x1; st.l22 = st.y0 - st.y1;
    st.l03 = q.l03[r]; st.l13 = q.l13[r]; st.l23 = q.l23[r];
    st.r1 = q.r1[r]; st.r2 = q.r2[r]; st.r3 = q.r3[r];
    st.fast = st.r1 != 0.0f;
    st.rej1 = st.rej2 = st.rej3 = 0.0f;
    return st;
}

// Flattened item index -> the record holding item p of the batch (`wo`: exclusive prefix of the wavefronts' totals)
CR_DEV int find_record(const uint32_t *scan, const uint32_t *wo, int p, uint32_t &first)
{
    int w = 0;
#pragma unroll
    for (int v = 1; v < kThreads / 64; ++v)
        if ((uint32_t)p >= wo[v]) w = v;
    const uint32_t pl = (uint32_t)p - wo[w];
    int lo = w * 64, n = 64;   // last slot in [lo, lo + 64) with scan <= pl
    while (n > 1) {
        const int half = n >> 1;
        if (scan[lo + half] <= pl) lo += half;
        n -= half;
    }
    first = pl - scan[lo];
    return lo;
}

// No pixel of [xa, xb] x [ya, yb] can hold a fragment: one edge is surely outside (raster_math.h (1)) at the corner
// where its numerator is largest.  Exact, never a guess (raster.hip, rect_surely_missed).
CR_DEV bool rect_surely_missed(const TriSetup &s, int xa, int xb, int ya, int yb)
{
    const float fxa = (float)xa, fxb = (float)xb, fya = (float)ya, fyb = (float)yb;
    auto worst = [&](float l1, float l2, float ya_, float xb_, float rej) {
        const float fy = (l1 * rej >= 0.0f) ? fyb : fya;
        const float fx = (l2 * rej >= 0.0f) ? fxa : fxb;
        return (l1 * (fy - ya_) - l2 * (fx - xb_)) * rej;
    };
    return worst(s.l01, s.l02, s.y2, s.x2, s.rej1) < -kRejTiny ||
           worst(s.l11, s.l12, s.y0, s.x0, s.rej2) < -kRejTiny ||
           worst(s.l21, s.l22, s.y1, s.x1, s.rej3) < -kRejTiny;
}

// Background of a rectangle, write-through (sc1: the clears leave the L2 to the lists, raster.hip clear_rect):
// full-width rows of 16-byte aligned planes as float4 stores, anything else pixel by pixel.
typedef float cr_v4f __attribute__((ext_vector_type(4)));
CR_DEV void st4(float *p, const float4 &v)
{
    const cr_v4f x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(x) : "memory");
}
CR_DEV void clear_rect(float *__restrict__ zb, float *__restrict__ cb, float *__restrict__ nb, int W,
                       int X0, int Y0, int X1, int Y1, bool vec, int tid)
{
    const size_t p0 = (size_t)Y0 * W + X0;
    float *z0 = zb + p0, *c0 = cb + p0 * 3, *n0 = nb + p0 * 3;
    const uint32_t t = (uint32_t)tid, uW = (uint32_t)W;
    float z1 = 1e6f, o1 = 0.0f;
    asm volatile("" : "+v"(z1), "+v"(o1));
    if (vec && X1 - X0 == TS) {
        const float4 zv = make_float4(z1, z1, z1, z1), ov = make_float4(o1, o1, o1, o1);
        constexpr uint32_t ZQ = TS / 4, CQ = 3 * TS / 4;          // float4 per row: z, colour / normal
        const uint32_t rows = (uint32_t)(Y1 - Y0);
        for (uint32_t i = t; i < rows * ZQ; i += kThreads) {
            const uint32_t r = i / ZQ, off = r * uW + (i - r * ZQ) * 4;
            st4(z0 + off, zv);
        }
        for (uint32_t i = t; i < rows * CQ; i += kThreads) {
            const uint32_t r = i / CQ, off = r * uW * 3 + (i - r * CQ) * 4;
            st4(c0 + off, ov);
            st4(n0 + off, ov);
        }
        return;
    }
    const uint32_t w = (uint32_t)(X1 - X0), n = w * (uint32_t)(Y1 - Y0);
    for (uint32_t p = t; p < n; p += kThreads) {
        const uint32_t dy = p / w, off = dy * uW + (p - dy * w);
        z0[off] = z1;
        c0[off * 3] = o1; c0[off * 3 + 1] = o1; c0[off * 3 + 2] = o1;
        n0[off * 3] = o1; n0[off * 3 + 1] = o1; n0[off * 3 + 2] = o1;
    }
}

// The launch's arguments: what this path reads, once.  The frame's geometry is S.G — a slot's two plans are alike
// (crender_pipeline_set_lookahead), and the host checks it.
struct Frame32Args {
    SetupArgs S;                 // the binning wavefronts of the slot's next frame, into its other plan
    int nsetup;
    const float *proj, *col, *nrm;
    float *zb, *cb, *nb;
    const uint32_t *count;       // list lengths of THIS frame (never written here)
    uint32_t *count_next;        // the other parity's counters: zeroed here for the next frame
    const float4 *bins;          // [ntiles][capacity] entries (BinEntry)
    uint32_t capacity, T;
    uint32_t *heavy_flag, *heavy_slots;      // null: the launch has no helper workgroups
    uint32_t *heavy_ctr_next, *hint_bad_next;
    int nhelp;
    uint32_t quad_at;
    int vec_clear;
    const uint32_t *hdr;
    uint32_t *usage;
    uint32_t usage_seq;
    uint32_t *stats, *stats_prev;
};

// One record of a tile's list; false: a stale index (beyond the frame's triangle count), no work.
// (the slab is at most kDirectBinBytes long: 32-bit byte offsets)
CR_DEV bool load_entry(const float4 *__restrict__ bins, uint32_t idx, uint32_t T, uint32_t &id, TriXYZ &t,
                       uint32_t &ebx, uint32_t &eby)
{
    const float4 *e = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(bins) + idx * (uint32_t)sizeof(BinEntry));
    const float4 e0 = e[0], e1 = e[1], e2 = e[2];
    t = TriXYZ{e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w, e2.x};
    id = __float_as_uint(e2.y);
    ebx = __float_as_uint(e2.z);
    eby = __float_as_uint(e2.w);
    return id < T;
}

// The run-wise sweep (raster.hip, sweep_runs32): the work items are pairs of x-neighbours of the clipped boxes'
// rows; thread t takes items [t c, (t + 1) c) of the batch, finds the record of its first item ONCE and walks:
// next pair, next row, next record — one flat loop stepped with selects.
CR_DEV void sweep_runs(const Queue &q, unsigned long long *key, const uint32_t *wo, int total, int tid, int X0, int Y0)
{
    const int chunk = (total + kThreads - 1) / kThreads;
    int e = tid * chunk;
    int left = (e + chunk < total ? e + chunk : total) - e;
    if (left <= 0) return;
    uint32_t i;
    int r = find_record(q.px_scan, wo, e, i);
    int dy, px0;
    {
        const int bwn = (packed_w(q.box[r]) + kItemPixels32 - 1) / kItemPixels32;
        // (i / bwn for i < 1024, bwn <= 16: the approximate reciprocal is exact enough)
        dy = (int)(((float)i + 0.5f) * __builtin_amdgcn_rcpf((float)bwn));
        px0 = ((int)i - dy * bwn) * kItemPixels32;
    }
    while (left > 0) {
        const uint32_t pb = q.box[r];
        const int bw = packed_w(pb), bh = packed_h(pb);
        const TriSetup st = queued_setup(q, r);
        const uint32_t id = q.tri[r];
        // tile-local pixel of the item's first sample; the samples speak frame coordinates
        const int lx = (int)(pb & 0x3Fu) + px0, ly = (int)((pb >> 6) & 0x3Fu) + dy;
#pragma unroll
        for (int j = 0; j < kItemPixels32; ++j) {
            float n1, n2, n3;
            numerators(st, X0 + lx + j, Y0 + ly, n1, n2, n3);
            unsigned long long k;
            if (fragment_from(st, id, n1, n2, n3, k) && px0 + j < bw)
                __hip_atomic_fetch_min(&key[key_slot(lx + j, ly)], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        left -= bw != 0 ? 1 : 0;
        px0 += kItemPixels32;
        const bool row_done = px0 >= bw;
        px0 = row_done ? 0 : px0;
        dy += row_done ? 1 : 0;
        const bool rec_done = dy >= bh;
        dy = rec_done ? 0 : dy;
        r += rec_done ? 1 + (int)packed_skip(pb) : 0;
    }
}

// The per-pixel resolve: every pixel of the rectangle is written exactly once, by plain stores of one, three and
// three words.  A part's pixels are taken in rows of its own width.
CR_DEV void resolve_tile(const Frame32Args &A, const Queue &q, const unsigned long long *key, int W,
                         int X0, int Y0, int X1, int Y1, int rw, int quad, uint32_t last_batch, int tid)
{
    const int npx = quad >= 0 ? rw * (TS / 2) : TS * TS;
    for (int p0 = tid; p0 < npx; p0 += kThreads) {
        const int dy = rw == TS ? p0 / TS : p0 / (TS / 2), dx = p0 - dy * rw;
        const int x = X0 + dx, y = Y0 + dy;
        if (x >= X1 || y >= Y1) continue;
        const uint32_t pix = (uint32_t)y * (uint32_t)W + (uint32_t)x;
        const uint32_t low = (uint32_t)key[key_slot(dx, dy)];
        if (low == KEY_LOW_PRIOR) {
            store_background<uint32_t>(pix, A.zb, A.cb, A.nb, nullptr);
            continue;
        }
        if constexpr (kSlotted) {
            const uint32_t id = 0xFFFFu - (low >> 16);
            if (((low >> 8) & 0xFFu) == last_batch) {
                // the winner's record is still in the queue: shade_and_store's operations on the same inputs
                // (.pyx:219, 226-242) with the quotients through the record's reciprocals (raster_math.h (2))
                const TriSetup st = queued_setup(q, (int)(low & 0xFFu));
                float c[9], n[9];
                load9(elem(A.col, (uint32_t)(id * 9u)), c);
                load9(elem(A.nrm, (uint32_t)(id * 9u)), n);
                float n1, n2, n3, b1, b2, b3;
                numerators(st, x, y, n1, n2, n3);
                quotients(st, n1, n2, n3, b1, b2, b3);
                store_fragment<uint32_t>(interp(st.z0, st.z1, st.z2, b1, b2, b3), c, n, b1, b2, b3,
                                         Light{0.f, 0.f, 0.f, 0}, pix, A.zb, A.cb, A.nb);
                continue;
            }
            shade_and_store<uint32_t>(A.proj, A.col, A.nrm, id, x, y, pix, A.zb, A.cb, A.nb);
        } else {
            shade_and_store<uint32_t>(A.proj, A.col, A.nrm, 0xFFFFFFFEu - low, x, y, pix, A.zb, A.cb, A.nb);
        }
    }
}

// The staged resolve: resolve_tile's pixels by the same operations, stored as whole rows, written through like the
// clear's.  For a rectangle of full width (X1 - X0 == rw) in a frame of 16-byte rows (A.vec_clear) the 64 pixels of
// one wavefront pass are whole rows of the rectangle — two of 32 pixels, four of 16 — and a row's bytes are
// contiguous and 16-byte aligned in each plane.  A thread ends a pass holding its pixel's seven words; the wavefront
// lays one plane's 64 pixels down in LDS in pixel order and reads them back 16 bytes per lane (take4): colour,
// normal, z, back to back through the same 768 bytes — a wavefront's LDS operations complete in order, so nothing
// waits between them — and only then the three 16-byte stores (st4o), 48 + 48 + 16 lanes.  (Store, then stage the
// next plane, is one LDS round trip per plane on every covered workgroup's critical path, and lost what the
// write-through gains: profiles/frame32/ab_writethrough.txt.)  The space is the wavefront's quarter of the queue's
// tri / box / px_scan arrays: behind the last sweep's barrier the resolve reads the queue's coordinates,
// denominators and reciprocals, nothing else.  No workgroup barrier.  A row at or below Y1 (a frame's cut bottom
// tile row) is shaded by nobody and stored by nobody.
static_assert(offsetof(Queue, box) == offsetof(Queue, tri) + 4 * kThreads &&
              offsetof(Queue, px_scan) == offsetof(Queue, box) + 4 * kThreads && offsetof(Queue, tri) % 16 == 0 &&
              3 * 4 * kThreads == (kThreads / 64) * 64 * 12, "64 pixels x 12 bytes of staging space per wavefront");

struct Pixel7 {
    float z, c0, c1, c2, n0, n1, n2;
};

// (base + a 32-bit byte offset, the base in scalar registers: elem()'s form of address)
CR_DEV void st4o(float *base, uint32_t byte_off, const float4 &v)
{
    const cr_v4f x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, %2 sc1" : : "v"(byte_off), "v"(x), "s"(base) : "memory");
}

// Staged words 4 * at .. 4 * at + 3: what every lane of the wavefront wrote before is read, and what is written
// next does not overtake the read (the fences order the compiler; the hardware needs no instruction for it).
CR_DEV float4 take4(const float *stg, int at)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float4 v = *reinterpret_cast<const float4 *>(stg + 4 * at);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return v;
}

CR_DEV void resolve_tile_rows(const Frame32Args &A, Queue &q, const unsigned long long *key, int W,
                              int X0, int Y0, int Y1, int rw, int quad, uint32_t last_batch, int tid)
{
    const int lane = tid & 63;
    float *stg = reinterpret_cast<float *>(q.tri) + (tid >> 6) * (64 * 3);
    const int npx = quad >= 0 ? rw * (TS / 2) : TS * TS;       // (a multiple of kThreads: every lane makes every pass)
    const int wave_rows = rw == TS ? 2 : 4;
    // lane j < 48 puts out words 4j .. 4j + 3 of a pass's colours and normals (24 or 12 lanes to a row), lane j < 16
    // those of its depths (8 or 4 lanes to a row); the other lanes read along (word 0) and store nothing
    const int rc = rw == TS ? lane / 24 : lane / 12, rz = rw == TS ? lane >> 3 : lane >> 2;
    const int at_c = lane < 48 ? lane : 0, at_z = lane < 16 ? lane : 0;
    const uint32_t uW = (uint32_t)W;
    const uint32_t in_c = (uint32_t)rc * (uW * 12u) + (uint32_t)(lane - rc * (rw == TS ? 24 : 12)) * 16u;
    const uint32_t in_z = (uint32_t)rz * (uW * 4u) + (uint32_t)(lane - rz * (rw == TS ? 8 : 4)) * 16u;
    for (int p0 = tid; p0 < npx; p0 += kThreads) {
        const int dy = rw == TS ? p0 / TS : p0 / (TS / 2), dx = p0 - dy * rw;
        const int x = X0 + dx, y = Y0 + dy;
        Pixel7 v{1e6f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};    // (store_background's words)
        const uint32_t low = (uint32_t)key[key_slot(dx, dy)];
        if (y < Y1 && low != KEY_LOW_PRIOR) {
            // resolve_tile's three cases, operation for operation; the words stay in registers
            const uint32_t id = kSlotted ? 0xFFFFu - (low >> 16) : 0xFFFFFFFEu - low;
            float c[9], n[9], b1, b2, b3;
            if (kSlotted && ((low >> 8) & 0xFFu) == last_batch) {
                const TriSetup st = queued_setup(q, (int)(low & 0xFFu));
                load9(elem(A.col, (uint32_t)(id * 9u)), c);
                load9(elem(A.nrm, (uint32_t)(id * 9u)), n);
                float n1, n2, n3;
                numerators(st, x, y, n1, n2, n3);
                quotients(st, n1, n2, n3, b1, b2, b3);
                v.z = interp(st.z0, st.z1, st.z2, b1, b2, b3);
            } else {
                const TriXYZ t = load_tri(elem(A.proj, (uint32_t)(id * 9u)));
                load9(elem(A.col, (uint32_t)(id * 9u)), c);
                load9(elem(A.nrm, (uint32_t)(id * 9u)), n);
                barycentric(t, x, y, b1, b2, b3);
                v.z = interp(t.z0, t.z1, t.z2, b1, b2, b3);
            }
            const Shade s = shade_fragment(c, n, b1, b2, b3, Light{0.f, 0.f, 0.f, 0});
            v.c0 = s.c0; v.c1 = s.c1; v.c2 = s.c2;
            v.n0 = s.n0; v.n1 = s.n1; v.n2 = s.n2;
        }
        // ---- the wavefront's rows: the first is row ya of the frame, its first pixel pixel `pix0`
        const int first = __builtin_amdgcn_readfirstlane(p0 - lane);       // (the wavefront's first pixel)
        const int ya = Y0 + (rw == TS ? first / TS : first / (TS / 2));
        const int rows_ok = Y1 - ya < wave_rows ? Y1 - ya : wave_rows;     // (<= 0: the whole pass is cut)
        const uint32_t pix0 = (uint32_t)ya * (uint32_t)W + (uint32_t)X0;
        const bool put_c = lane < 48 && rc < rows_ok, put_z = lane < 16 && rz < rows_ok;
        stg[lane * 3] = v.c0; stg[lane * 3 + 1] = v.c1; stg[lane * 3 + 2] = v.c2;
        const float4 c4 = take4(stg, at_c);
        stg[lane * 3] = v.n0; stg[lane * 3 + 1] = v.n1; stg[lane * 3 + 2] = v.n2;
        const float4 n4 = take4(stg, at_c);
        stg[lane] = v.z;
        const float4 z4w = take4(stg, at_z);
        if (put_c) {
            st4o(A.cb, pix0 * 12u + in_c, c4);
            st4o(A.nb, pix0 * 12u + in_c, n4);
        }
        if (put_z) st4o(A.zb, pix0 * 4u + in_z, z4w);
    }
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kWavesPerSimd32)))
void k_frame32(Frame32Args A)
{
    __shared__ __attribute__((aligned(16))) unsigned long long key[TS * TS];
    __shared__ __attribute__((aligned(16))) unsigned char qraw[sizeof(Queue)];
    if ((int)blockIdx.x < A.nsetup) {
        if (threadIdx.x < kWave)
            setup_wave_body<TS, true>(A.S.tri_in, A.S.nrm, A.S.proj_out, A.S.count, A.S.bins, A.S.dcap, A.S.hdr,
                                      A.S.hv, A.S.T, A.S.P, A.S.G, (int64_t)blockIdx.x, qraw);
        return;
    }
    Queue &q = *reinterpret_cast<Queue *>(qraw);
    const Geom &G = A.S.G;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = (int)blockIdx.x - A.nsetup;

    // ---- which tile, and which part of it: [3 * hmax helpers][ntiles main workgroups]
    const bool helper = b < A.nhelp;
    int tile, quad = -1;           // -1 = the whole tile, 0..3 = one part of a heavy tile (half or quadrant)
    if (helper) {
        const uint32_t v = A.heavy_slots[b];
        if (v == 0) return;                              // (same word for every thread: uniform)
        tile = (int)v - 1;
        quad = 1 + b % 3;
    } else {
        const int m = b - A.nhelp;
        if (m == 0 && tid == 0) {
            *A.heavy_ctr_next = 0;
            *A.hint_bad_next = 0;
        }
        if (m == G.ntiles - 1 && tid == 0) {
            // (the binning pass that wrote the header ran in an earlier launch of the stream; so did the launch
            // that counted into stats_prev)
            uint32_t nl = 0, ns = 0;
            constexpr int kQuads = kStatWords / 4;      // a parity's (large, small) pairs, four words at a time
            uint4 v[kQuads];
#pragma unroll
            for (int i = 0; i < kQuads; ++i) v[i] = reinterpret_cast<const uint4 *>(A.stats_prev)[i];
#pragma unroll
            for (int i = 0; i < kQuads; ++i) {
                nl += v[i].x + v[i].z; ns += v[i].y + v[i].w;
                reinterpret_cast<uint4 *>(A.stats_prev)[i] = make_uint4(0u, 0u, 0u, 0u);
            }
            uint4 *rec = reinterpret_cast<uint4 *>(A.usage);
            rec[1] = make_uint4(nl, ns, 0u, A.usage_seq);          // (kernel: the general path's number)
            rec[0] = make_uint4(A.usage_seq, A.hdr[kHdrEntriesLo], A.hdr[kHdrOverflow], A.hdr[kHdrEntriesHi]);
        }
        // raster order, row ty rotated by 9 * ty columns (raster.hip, pick_tile: every (XCD, engine) pair walks
        // through every tile column)
        const int ty = G.ntx_magic ? (int)__umulhi((uint32_t)m, G.ntx_magic) : m / G.ntx;
        const int t = m - ty * G.ntx + 9 * ty;
        const int tx = G.ntx_magic ? t - (int)__umulhi((uint32_t)t, G.ntx_magic) * G.ntx : t % G.ntx;
        tile = ty * G.ntx + tx;
    }
    const int ty = G.ntx_magic ? (int)__umulhi((uint32_t)tile, G.ntx_magic) : tile / G.ntx;
    const int tx = tile - ty * G.ntx;
    int X0 = tx * TS, Y0 = G.y0 + ty * TS;
    int X1 = (X0 + TS < G.W) ? (X0 + TS) : G.W;
    int Y1 = (Y0 + TS < G.y1) ? (Y0 + TS) : G.y1;

    // a main workgroup's two words, the list's length and the tile's split flag, are independent: both loads are
    // issued before either is waited for (a launch without helpers reads the length twice)
    const bool flagged = !helper && A.heavy_flag;
    const uint32_t *flag_at = flagged ? A.heavy_flag + tile : A.count + tile;
    uint32_t nlist = A.count[tile], flag = *flag_at;
    asm volatile("" : "+v"(nlist), "+v"(flag));          // (both words here: the second load is not sunk to its use)
    nlist = (uint32_t)__builtin_amdgcn_readfirstlane((int)nlist);
    flag = (uint32_t)__builtin_amdgcn_readfirstlane((int)flag);
    const uint32_t beg = (uint32_t)tile * A.capacity;
    const uint32_t end = beg + (nlist < A.capacity ? nlist : A.capacity);
    if (!helper) {
        if (flagged && flag) quad = 0;
        if (tid == 0) A.count_next[tile] = 0;            // the other parity's counter: zero for the next frame
    }
    int rw = TS;                 // width of this workgroup's rectangle in the key plane's terms
    if (quad >= 0) {
        constexpr int HS = TS / 2;
        if (end - beg >= A.quad_at) {           // four quadrants
            X0 += (quad & 1) * HS; Y0 += (quad >> 1) * HS;
            if (X1 > X0 + HS) X1 = X0 + HS;
            rw = HS;
        } else {                                // two halves; parts 2 and 3 have nothing to do
            if (quad >= 2) {
                if (tid == 0) A.heavy_slots[b] = 0;
                return;
            }
            Y0 += quad * HS;
        }
        if (Y1 > Y0 + HS) Y1 = Y0 + HS;
        if (X1 < X0) X1 = X0;
        if (Y1 < Y0) Y1 = Y0;
    }

    const bool work = beg != end && X0 < X1 && Y0 < Y1;     // (uniform over the workgroup)
    if (!work) {
        if (X0 < X1 && Y0 < Y1) clear_rect(A.zb, A.cb, A.nb, G.W, X0, Y0, X1, Y1, A.vec_clear && quad < 0, tid);
    } else {
        // first batch of the list straight into registers; the key plane's start value is a constant, written
        // while those loads are on their way and ordered by the queue's barrier (an empty tile never gets here)
        uint32_t cur_id = 0, cur_bx = 0, cur_by = 0;
        TriXYZ cur_t{};
        bool cur_ok = beg + (uint32_t)tid < end;
        if (cur_ok) cur_ok = load_entry(A.bins, beg + (uint32_t)tid, A.T, cur_id, cur_t, cur_bx, cur_by);
        {
            const unsigned long long key_clear = make_key(zord(1e6f), KEY_LOW_PRIOR);
#pragma unroll
            for (int p = tid; p < TS * TS; p += kThreads) key[p] = key_clear;
        }
        int tile_class = -1;         // (wavefront 0 learns it with the first batch, reports it last)
        for (uint32_t base = beg; base < end; base += kThreads) {
            // ---- queue this batch: one record per thread, slot = thread index
            uint32_t box_xy = 0, box_wh = 0;
            if (cur_ok) {
                int xl = (int)(cur_bx & 0xFFFF), xr = (int)(cur_bx >> 16);
                int yt = (int)(cur_by & 0xFFFF), yb = (int)(cur_by >> 16);
                if (xl < X0) xl = X0;
                if (xr > X1) xr = X1;
                if (yt < Y0) yt = Y0;
                if (yb > Y1) yb = Y1;
                if (xl < xr && yt < yb) {
                    box_xy = (uint32_t)xl | ((uint32_t)yt << 16);
                    box_wh = (uint32_t)(xr - xl) | ((uint32_t)(yb - yt) << 16);
                    // a large triangle's box covers about twice its area: the exact test on (box ∩ rectangle),
                    // not worth its ~80 instructions for a small box
                    if ((xr - xl) * (yb - yt) >= 256 && rect_surely_missed(make_setup(cur_t, false), xl, xr - 1, yt, yb - 1))
                        box_wh = 0;
                }
            }
            const int bw = (int)(box_wh & 0xFFFF), bh = (int)(box_wh >> 16);
            const uint32_t my_px = (uint32_t)(((bw + kItemPixels32 - 1) / kItemPixels32) * bh);
            if (base == beg && wave == 0) {
                // the tile's size class for the next frames' choice of kernel: is the first wavefront's share of
                // the list, on average, records of 16 blocks and more (0) or smaller ones (1)?
                const uint32_t incl_blocks = wave_incl_sum((uint32_t)(((bw + 3) >> 2) * ((bh + 3) >> 2)));
                const uint32_t tot0 = (uint32_t)__builtin_amdgcn_readlane((int)incl_blocks, 63);
                const uint32_t n0 = end - beg < 64u ? end - beg : 64u;
                tile_class = tot0 >= 16u * n0 ? 0 : 1;
            }
            const uint32_t incl_px = wave_incl_sum(my_px);
            const uint32_t batch = ((base - beg) / (uint32_t)kThreads) & 0xFFu;
            const uint32_t key_low = kSlotted ? ((0xFFFFu - (cur_id & 0xFFFFu)) << 16) | (batch << 8) | (uint32_t)tid
                                              : 0xFFFFFFFEu - cur_id;
            // the previous batch's sweep must be over before the queue is overwritten
            if (base != beg) __syncthreads();
            q.x0[tid] = cur_t.x0; q.y0[tid] = cur_t.y0; q.z0[tid] = cur_t.z0;
            q.x1[tid] = cur_t.x1; q.y1[tid] = cur_t.y1; q.z1[tid] = cur_t.z1;
            q.x2[tid] = cur_t.x2; q.y2[tid] = cur_t.y2; q.z2[tid] = cur_t.z2;
            q.tri[tid] = 0xFFFFFFFEu - key_low;
            {
                const unsigned long long live = __builtin_amdgcn_ballot_w64(box_wh != 0);
                const unsigned long long after = lane == 63 ? 0ull : live >> (lane + 1);
                const uint32_t skip = after ? (uint32_t)__builtin_ctzll(after) : (uint32_t)(63 - lane);
                q.box[tid] = pack_box(box_xy, box_wh, X0, Y0) | (skip << 26);
            }
            if (box_wh != 0) {
                const TriSetup mine = make_setup(cur_t, true);
                q.l03[tid] = mine.l03; q.l13[tid] = mine.l13; q.l23[tid] = mine.l23;
                q.r1[tid] = mine.fast ? mine.r1 : 0.0f; q.r2[tid] = mine.r2; q.r3[tid] = mine.r3;
            }
            q.px_scan[tid] = incl_px - my_px;
            if (lane == 63) q.wave_px[wave] = incl_px;
            __syncthreads();  // queue (and, for the first batch, key plane) complete

            uint32_t wo[kThreads / 64 + 1];
            wo[0] = 0;
#pragma unroll
            for (int w = 0; w < kThreads / 64; ++w) wo[w + 1] = wo[w] + q.wave_px[w];
            // next batch: issue its loads now, they complete under the sweep
            const uint32_t nxt = base + (uint32_t)kThreads + (uint32_t)tid;
            cur_ok = nxt < end;
            if (cur_ok) cur_ok = load_entry(A.bins, nxt, A.T, cur_id, cur_t, cur_bx, cur_by);
            sweep_runs(q, key, wo, (int)wo[kThreads / 64], tid, X0, Y0);
        }
        __syncthreads();
        const uint32_t last_batch = ((end - beg - 1) / (uint32_t)kThreads) & 0xFFu;
        if (kRowStores && A.vec_clear && X1 - X0 == rw)         // (uniform over the workgroup)
            resolve_tile_rows(A, q, key, G.W, X0, Y0, Y1, rw, quad, last_batch, tid);
        else
            resolve_tile(A, q, key, G.W, X0, Y0, X1, Y1, rw, quad, last_batch, tid);
        // one covered tile's size class into the frame's statistics: one lane, its last memory operation
        if (tid == 0 && tile_class >= 0)
            atomicAdd(&A.stats[(((blockIdx.x >> 3) & (kStatWords / 2 - 1)) << 1) + (uint32_t)tile_class], 1u);
    }
    // hand-off words of a heavy tile go back to zero once every wavefront has read them
    if (quad >= 0) {
        __syncthreads();
        if (tid == 0) {
            if (!helper) A.heavy_flag[tile] = 0;
            else A.heavy_slots[b] = 0;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------
std::mutex g_lock;
std::unordered_map<const crender_pipeline *, bool> g_last;      // crender_frame32_last

void note_last(const crender_pipeline *p, bool took)
{
    std::lock_guard<std::mutex> hold(g_lock);
    g_last[p] = took;
}

// The raster pass of a look-ahead frame: the small-scene kernel where the frame qualifies, with everything
// run_raster_pass<32> (raster.hip) does to the plan on the host; any other frame goes to raster_pass unchanged.
int frame32_raster_pass(crender_plan *plan, const float *d_col, const float *d_nrm, int64_t T, float *d_z,
                        float *d_color, float *d_normal, int32_t *d_winner, unsigned flags, hipStream_t s,
                        const SetupArgs *with_setup, bool *took)
{
    *took = false;
    const Layout &L = plan->L;
    const Geom &G = L.g;
    raster_path_hint(plan);          // (raster_pass asks again: nothing newer is there then, same answer)
    const unsigned need = CRENDER_FUSED_CLEAR | CRENDER_OVERLAPPED_FRAMES;
    bool ok = with_setup && L.ts == TS && plan->last_frame_mode == kFrameDirect && T > 0 && T == plan->last_T &&
              (flags & need) == need && !(flags & CRENDER_FUSED_GURO) && !d_winner && d_z && d_color && d_normal &&
              d_col && d_nrm && !plan->orig_of && !plan->pos_of && !plan->normal_z && !plan->frame_lone &&
              plan->forced_path < 0 && default_raster_path() < 0 && plan->auto_path == 0 /* the general kernel */;
    // 32-bit offsets, slotted keys, the identity tile map (raster order; large grids are scattered)
    ok = ok && (uint64_t)G.H * (uint64_t)G.W * 12ull < (1ull << 32) && T <= kDirectMaxTriangles &&
         G.ntiles < 32768 && L.direct_cap > 0 && L.direct_cap <= 256 * (int64_t)kThreads;
    if (ok) {
        // a slot's two plans are alike: the launch reads ONE geometry
        const Geom &B = with_setup->G;
        ok = B.W == G.W && B.H == G.H && B.y0 == G.y0 && B.y1 == G.y1 && B.ntx == G.ntx && B.nty == G.nty &&
             B.ntiles == G.ntiles && B.ntx_magic == G.ntx_magic;
    }
    if (!ok)
        return raster_pass(plan, plan->proj(), d_col, d_nrm, T, d_z, d_color, d_normal, d_winner, flags, s, with_setup);

    const int par = plan->parity;
    const bool split = plan->frame_hmax > 0;
    Frame32Args A;
    A.S = *with_setup;
    A.nsetup = (int)((with_setup->T + kWave - 1) / kWave);
    A.proj = plan->proj(); A.col = d_col; A.nrm = d_nrm;
    A.zb = d_z; A.cb = d_color; A.nb = d_normal;
    A.count = plan->count(par);
    A.count_next = plan->count(par ^ 1);
    A.bins = plan->direct();
    A.capacity = (uint32_t)L.direct_cap;
    A.T = (uint32_t)plan->last_T;
    A.heavy_flag = split ? plan->hflag() : nullptr;
    A.heavy_slots = split ? plan->hslots() : nullptr;
    A.heavy_ctr_next = plan->heavy_ctr(par ^ 1);
    A.hint_bad_next = plan->hint_bad(par ^ 1);
    A.nhelp = split ? 3 * plan->frame_hmax : 0;
    A.quad_at = plan->frame_quad_at;
    const uintptr_t any = (uintptr_t)d_z | (uintptr_t)d_color | (uintptr_t)d_normal;
    A.vec_clear = (any & 15u) == 0 && (G.W & 3) == 0;
    plan->last_ordered = false;          // (frames in flight are never ordered)
    plan->last_path = 0;
    // this launch's usage record (crender_plan_poll_bin_usage)
    plan->ticket++;
    const int uslot = (int)(plan->ticket % kUsageRing);
    plan->usage_mode[uslot] = plan->last_frame_mode;
    A.hdr = plan->hdr();
    A.usage = plan->usage_dev + kUsageWords * uslot;
    A.usage_seq = (uint32_t)plan->ticket ^ plan->usage_salt;
    A.stats = plan->stats((int)(plan->ticket & 1u));
    A.stats_prev = plan->stats((int)((plan->ticket & 1u) ^ 1u));
    plan->awaiting[par ^ 1] = false;     // zeroed by this launch
    plan->unrastered[par] = false;
    const unsigned grid = (unsigned)(A.nsetup + A.nhelp + G.ntiles);
    hipLaunchKernelGGL(k_frame32, dim3(grid), dim3(kThreads), 0, s, A);
    CR_LAUNCH_CHECK("k_frame32");
    *took = true;
    return CRENDER_OK;
}

}  // namespace

extern "C" {

int crender_frame32_submit(crender_pipeline *p, void *stream)
{
    if (!p) return fail(CRENDER_EINVAL, "null pipeline");
    const int k = (int)(p->n % (uint64_t)p->depth);
    const crender_pipeline::Bound &b = p->bound[k];
    if (!b.set) return fail(CRENDER_EINVAL, "crender_pipeline_submit: slot not bound");
    const unsigned need = CRENDER_FUSED_CLEAR | CRENDER_OVERLAPPED_FRAMES;
    // what can be told without touching the pipeline: anything else is crender_pipeline_submit's, unchanged
    if (!p->ahead[k] || !b.has_P || b.T <= 0 || b.winner || !b.z || !b.color || !b.normal || !b.col ||
        (b.flags & need) != need || (b.flags & CRENDER_FUSED_GURO) || p->plan[k]->L.ts != TS) {
        note_last(p, false);
        return crender_pipeline_submit(p, stream);
    }
    // ---- the look-ahead branch of crender_pipeline_frame (abi.hip), with frame32_raster_pass for raster_pass
    const float *d_tri = b.tri, *d_nrm = b.nrm, *P16 = b.P;
    const int64_t T = b.T;
    const unsigned flags = b.flags;
    hipStream_t caller = static_cast<hipStream_t>(stream);
    if (!p->synced || d_tri != p->last_tri || d_nrm != p->last_nrm || T != p->last_T || caller != p->last_caller) {
        // new inputs, or the first frame after a join: whatever produced the inputs, and whatever touched the
        // framebuffers last, was enqueued on the caller's stream
        if (hipStreamQuery(caller) != hipSuccess) {
            CR_HIP(hipEventRecord(p->mark, caller));
            for (int j = 0; j < p->depth; ++j) CR_HIP(hipStreamWaitEvent(p->s[j], p->mark, 0));
        }
        p->last_tri = d_tri; p->last_nrm = d_nrm; p->last_T = T; p->last_caller = caller;
        p->synced = true;
    }
    {   // the chain's plans share what any of them has learnt about the frames' size class
        crender_plan *use = p->sel[k] ? p->ahead[k] : p->plan[k];
        if (raster_path_hint(use)) { p->shared_path = use->auto_path; p->shared_known = true; }
        else if (p->shared_known) { use->auto_path = p->shared_path; use->auto_known = true; }
    }
    const bool timed = p->timing();
    if (timed) CR_HIP(hipEventRecord(p->events[(size_t)p->timed_frames * 2], p->s[k]));
    crender_plan *cur = p->sel[k] ? p->ahead[k] : p->plan[k];
    crender_plan *nxt = p->sel[k] ? p->plan[k] : p->ahead[k];
    crender_pipeline::Primed &pr = p->primed[k];
    const bool have = pr.ok && pr.tri == d_tri && pr.nrm == d_nrm && pr.T == T && pr.flags == flags &&
                      std::memcmp(pr.P, P16, sizeof pr.P) == 0;
    pr.ok = false;
    int rc = CRENDER_OK;
    if (!have) rc = bin_pass(cur, true, d_tri, d_nrm, T, P16, flags, p->s[k]);
    SetupArgs sa;
    bool deferred = false, took = false;
    if (rc == CRENDER_OK) rc = bin_pass(nxt, true, d_tri, d_nrm, T, P16, flags, p->s[k], &sa, &deferred);
    if (rc == CRENDER_OK)
        rc = frame32_raster_pass(cur, b.col, d_nrm, T, b.z, b.color, b.normal, b.winner, flags, p->s[k],
                                 deferred ? &sa : nullptr, &took);
    note_last(p, took);
    if (rc != CRENDER_OK) return rc;
    pr.ok = true; pr.tri = d_tri; pr.nrm = d_nrm; pr.T = T; pr.flags = flags;
    std::memcpy(pr.P, P16, sizeof pr.P);
    p->sel[k] ^= 1;
    p->n++;
    if (timed) {
        CR_HIP(hipEventRecord(p->events[(size_t)p->timed_frames * 2 + 1], p->s[k]));
        p->timed_frames++;
    }
    return CRENDER_OK;
}

int crender_frame32_last(const crender_pipeline *p)
{
    if (!p) return 0;
    std::lock_guard<std::mutex> hold(g_lock);
    auto it = g_last.find(p);
    return it != g_last.end() && it->second ? 1 : 0;
}

}  // extern "C"
