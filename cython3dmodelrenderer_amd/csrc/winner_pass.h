// winner_pass.h — what every deferred pass over the winner plane shares (texture.hip, texmip.hip, texaniso.hip,
// shadow.hip): a lane's pixel of an 8 x 8 block and its winner, the gather of the winner's corners, the store with
// the fused light, the texel fetches, and on the host the launch geometry, the light and the common argument
// checks.  Each translation unit gets its own copy (anonymous namespace); include after common.h and
// `using namespace crender_detail;`.
#pragma once

namespace {

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

// The three corners of triangle t, unprojected.
CR_DEV void gather_corners(const float *__restrict__ tri, int64_t t, float a[3], float b[3], float c[3])
{
    const float *v = tri + t * 9;
    a[0] = v[0]; a[1] = v[1]; a[2] = v[2];
    b[0] = v[3]; b[1] = v[4]; b[2] = v[5];
    c[0] = v[6]; c[1] = v[7]; c[2] = v[8];
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

// The argument checks every pass makes in these words; what else a pass takes it checks itself.
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

}  // namespace
