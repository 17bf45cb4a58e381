// winner_pass.h — what the deferred passes over the winner plane share (texture.hip, texmip.hip and texaniso.hip, the
// last two also through mip_sample.h; shadow.hip, phong.hip, ao.hip, wireframe.hip, bloom.hip, peel.hip, dof.hip,
// normal_map.hip, envmap.hip, motion.hip): the winner's triangle projected and the host's frame checks, then what the per-pixel
// passes share, then what the neighbourhood passes share.  Each translation unit gets its own copy (anonymous
// namespace); include after common.h and `using namespace crender_detail;`.
#pragma once

namespace {

// The three corners of triangle t, unprojected.
CR_DEV void gather_corners(const float *__restrict__ tri, int64_t t, float a[3], float b[3], float c[3])
{
    const float *v = tri + t * 9;
    a[0] = v[0]; a[1] = v[1]; a[2] = v[2];
    b[0] = v[3]; b[1] = v[4]; b[2] = v[5];
    c[0] = v[6]; c[1] = v[7]; c[2] = v[8];
}

// Triangle t on the screen: its corners gathered and projected.  `raw` keeps them unprojected, for what a pass blends.
CR_DEV TriXYZ winner_triangle(const float *__restrict__ tri, int64_t t, const ProjConst &P, float raw[3][3])
{
    gather_corners(tri, t, raw[0], raw[1], raw[2]);
    float a[3] = {raw[0][0], raw[0][1], raw[0][2]}, b[3] = {raw[1][0], raw[1][1], raw[1][2]},
          c[3] = {raw[2][0], raw[2][1], raw[2][2]};
    project_vertex(P, a);
    project_vertex(P, b);
    project_vertex(P, c);
    return TriXYZ{a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]};
}

CR_DEV TriXYZ winner_triangle(const float *__restrict__ tri, int64_t t, const ProjConst &P)
{
    float raw[3][3];
    return winner_triangle(tri, t, P, raw);
}

// fail() for a bad argument of `entry`: "<entry>: <what>".
inline int arg_error(const char *entry, const char *what)
{
    return fail(CRENDER_EINVAL, (std::string(entry) + ": " + what).c_str());
}

// The frame checks the passes make in these words and in this order; CRENDER_OK or the failure.  `have_tri`: the
// triangle arrays the entry needs with T > 0 are given.  The rows are apart: an entry may check more before them, or take none.
inline int frame_checks(const char *entry, int64_t T, bool have_tri, int H, int W, const char *no_tri = "d_tri is NULL with T > 0")
{
    if (T < 0) return arg_error(entry, "T is negative");
    if (T > 0 && !have_tri) return arg_error(entry, no_tri);
    if (H < 1 || W < 1) return arg_error(entry, "H or W is below 1");
    return CRENDER_OK;
}

inline int rows_check(const char *entry, int H, int y0, int y1)
{
    return (y0 < 0 || y1 > H || y0 >= y1) ? arg_error(entry, "rows outside the frame") : CRENDER_OK;
}

// P16 has crender_projection_matrix's shape: what a pass that rebuilds view depths from the z plane relies on.
inline int projection_shape_check(const char *entry, const float *P16)
{
    for (int i : {1, 2, 4, 6, 8, 9, 12, 13})
        if (!(P16[i] == 0.0f))
            return arg_error(entry, "P16 is not of crender_projection_matrix's shape (an entry that must be 0 is not)");
    for (int i : {0, 5, 14})
        if (!std::isfinite(P16[i]) || P16[i] == 0.0f)       // <cmath>'s, which common.h brings to every unit
            return arg_error(entry, "P16 is not of crender_projection_matrix's shape (entry 0, 5 or 14 is 0 or not finite)");
    return CRENDER_OK;
}

// ---- per-pixel passes ---------------------------------------------------------------------------------------------

constexpr int kPassBlock = 8;        // pixels along each side of a wavefront's block

// A lane's pixel: a workgroup is four wavefronts side by side (32 x 8 pixels), blockIdx.x counts them across the
// frame and `rb` is the row block, which the kernels step by gridDim.y.
struct WinnerPixel {
    int x, y;
    bool inside;                     // on the frame and above y1
    bool covered;                    // a triangle won it, and d_tri holds that triangle
    size_t pix;                      // y * W + x
    int64_t orig, t;                 // the winner in the caller's order (uv, ltri), and where it sits in d_tri
};

CR_DEV WinnerPixel winner_pixel(const int32_t *__restrict__ win, int64_t T, const uint32_t *__restrict__ pos_of, int W,
                                int y0, int y1, int rb)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WinnerPixel p;
    p.x = ((int)blockIdx.x * (kThreads / 64) + wave) * kPassBlock + (lane & (kPassBlock - 1));
    p.y = y0 + rb * kPassBlock + (lane >> 3);
    p.inside = p.x < W && p.y < y1;
    p.pix = (size_t)p.y * (size_t)W + (size_t)p.x;
    p.orig = -1;
    if (p.inside) p.orig = win[p.pix];
    p.covered = p.orig >= 0 && p.orig < T;
    p.t = p.orig;
    if (p.covered && pos_of) {
        p.t = pos_of[p.orig];
        p.covered = p.t < T;
    }
    return p;
}

// The end of a texture pass: `col` is the texture's colour of a covered pixel.  With the light every pixel of the
// frame is stored, an uncovered one from its own colour; without it only the covered ones.
template <bool LIGHT>
CR_DEV void store_shaded(const WinnerPixel &p, float col[3], const float *__restrict__ nb, const Light &L,
                         float *__restrict__ cb)
{
    if (LIGHT) {
        if (!p.inside) return;
        float *cp = cb + p.pix * 3;
        const float *np_ = nb + p.pix * 3;
        if (!p.covered) { col[0] = cp[0]; col[1] = cp[1]; col[2] = cp[2]; }
        const float f = guro_factor(L, np_[0], np_[1], np_[2]);
        cp[0] = col[0] * f; cp[1] = col[1] * f; cp[2] = col[2] * f;
    } else if (p.covered) {
        float *cp = cb + p.pix * 3;
        cp[0] = col[0]; cp[1] = col[1]; cp[2] = col[2];
    }
}

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

// The Bilinear statement of crender_tex.h on one texture or one level of a chain.
CR_DEV void bilinear(const unsigned char *__restrict__ tex, int th, int tw, float tu, float tv, float c[3])
{
    const float fx = tu * (float)tw - 0.5f, fy = (1.0f - tv) * (float)th - 0.5f;
    const float x0 = floorf(fx), yf0 = floorf(fy);
    const float ax = fx - x0, ay = fy - yf0;
    const int cl = clipi(host_f32_to_i32(x0), 0, tw - 1), cr = clipi(host_f32_to_i32(x0 + 1.0f), 0, tw - 1);
    const int rt = clipi(host_f32_to_i32(yf0), 0, th - 1), rbm = clipi(host_f32_to_i32(yf0 + 1.0f), 0, th - 1);
    const unsigned char *t00 = texel(tex, rt, cl, tw), *t01 = texel(tex, rt, cr, tw);
    const unsigned char *t10 = texel(tex, rbm, cl, tw), *t11 = texel(tex, rbm, cr, tw);
    const float wx = 1.0f - ax, wy = 1.0f - ay;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        c[j] = ((float)t00[j] * wx + (float)t01[j] * ax) * wy + ((float)t10[j] * wx + (float)t11[j] * ax) * ay;
}

// The launch geometry of rows [y0, y1) of a frame W wide: a workgroup per 32 x 8 pixels, and no more row blocks
// in the grid than a grid may be tall (the kernels loop over the rest).
struct PassGrid {
    int row_blocks;
    dim3 grid;
};

inline PassGrid pass_grid(int W, int y0, int y1)
{
    const int row_blocks = (y1 - y0 + kPassBlock - 1) / kPassBlock;
    const int across = kPassBlock * (kThreads / 64);
    return {row_blocks, dim3((unsigned)((W + across - 1) / across), (unsigned)(row_blocks < 65535 ? row_blocks : 65535))};
}

inline Light pass_light(const float *light3)
{
    return light3 ? Light{light3[0], light3[1], light3[2], 1} : Light{0.0f, 0.0f, 0.0f, 0};
}

// The argument checks of the texture passes, which report them all in one message; what else a pass takes it checks itself.
inline bool frame_args_ok(const int32_t *d_winner, const float *P16, const float *d_color, int64_t T, const float *d_tri,
                          int H, int W, int y0, int y1)
{
    return d_winner && P16 && d_color && T >= 0 && (T == 0 || d_tri) && H >= 1 && W >= 1 && y0 >= 0 && y1 <= H && y0 < y1;
}

// and the pairing of the fused light with the normal plane
inline bool light_args_ok(const float *light3, const float *d_normal)
{
    return (light3 != nullptr) == (d_normal != nullptr);
}

// ---- neighbourhood passes -----------------------------------------------------------------------------------------
// A workgroup owns a tile of kTile x kTile pixels and stages what its taps read of the tile plus a halo of R pixels on
// every side into LDS, [kTile + 2R][kTile + 2R] words.  256 work items are 32 x 8 pixels, a wavefront two rows of 32.

constexpr int kTile = 32;                       // pixels along each side of a workgroup's tile
constexpr int kTileRows = kThreads / kTile;     // rows of it the 256 work items cover at a time

// A work item's place: in its wavefront, which stages a row at a time, and in the 32 x 8 pixels.
struct TileLane { int lane, wave, lx, ly; };

CR_DEV TileLane tile_lane()
{
    return {(int)(threadIdx.x & 63), (int)(threadIdx.x >> 6), (int)(threadIdx.x & (kTile - 1)), (int)(threadIdx.x >> 5)};
}

// The first pixel (x0, ty0) of tile `tile` of a strip that starts at row y0, tiles_x tiles across.
struct TileOrigin { int x0, ty0; };

CR_DEV TileOrigin tile_origin(int tile, int tiles_x, int y0)
{
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    return {tx * kTile, y0 + ty * kTile};
}

// The tiles of rows [y0, y1) of a frame W wide: tiles_x across and `tiles` in all; the failure if a grid cannot count them.
inline int tile_grid(const char *entry, int W, int y0, int y1, int &tiles_x, int &tiles)
{
    tiles_x = (W + kTile - 1) / kTile;
    const int64_t n = (int64_t)tiles_x * (int64_t)((y1 - y0 + kTile - 1) / kTile);
    if (n > 0x7FFFFFFF) return arg_error(entry, "H or W is too large");
    tiles = (int)n;
    return CRENDER_OK;
}

// The bytes of LDS of a tile staged with a halo of R, and `more` words after it.
inline size_t tile_lds_bytes(int R, int more = 0)
{
    return (size_t)((kTile + 2 * R) * (kTile + 2 * R) + more) * 4;
}

}  // namespace
