// mip_sample.h — what the two texture passes over a mip chain share (texmip.hip: trilinear; texaniso.hip:
// anisotropic): the chain's layout, one bilinear sample of a level, and (u, v) of an integer pixel through
// raster_math.h's TriSetup.  Each translation unit gets its own copy (anonymous namespace); include after
// common.h and crender_mip.h.
#pragma once

namespace {

constexpr int kTexBlock = 8;         // pixels along each side of a wavefront's block
constexpr int kMaxLevels = CRENDER_MIP_MAX_LEVELS;

// Where each level starts in the chain, by value in the kernel's arguments; a level's height and width are
// shifts of the texture's (h_k = max(1, th >> k)).
struct MipChain {
    unsigned long long off[kMaxLevels];
    int th, tw, L;
};

// The chain's shape; false for a texture crender_mip_layout refuses.
bool chain_layout(int th, int tw, int &L, int h[kMaxLevels], int w[kMaxLevels], unsigned long long off[kMaxLevels],
                  unsigned long long &total)
{
    if (th < 1 || tw < 1 || th > 65535 || tw > 65535) return false;
    const int side = th > tw ? th : tw;
    L = 0;
    while ((side >> L) > 0) ++L;     // 1 + floor(log2(side))
    total = 0;
    for (int k = 0; k < kMaxLevels; ++k) {
        const bool in = k < L;
        h[k] = in ? ((th >> k) > 1 ? (th >> k) : 1) : 0;
        w[k] = in ? ((tw >> k) > 1 ? (tw >> k) : 1) : 0;
        off[k] = in ? total : 0;
        total += 3ull * (unsigned long long)h[k] * (unsigned long long)w[k];
    }
    return true;
}

// The host's truncating float -> int32 conversion (cvttss2si): INT_MIN for a NaN and out of range.
// (Restated from model_ops.hip, whose text is fingerprinted, as texture.hip restates it.)
CR_DEV int host_f32_to_i32(float f)
{
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : (int)0x80000000;
}

CR_DEV const unsigned char *texel(const unsigned char *__restrict__ tex, int row, int colm, int tw)
{
    return tex + ((size_t)row * (size_t)tw + (size_t)colm) * 3;
}

// The Bilinear statement of crender_tex.h on one level (texture.hip's operation order).
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

struct CornerUV {
    float u0, v0, u1, v1, u2, v2;
    float za, zb, zc;                // the corners' unprojected z (perspective mode)
    float ra, rb, rc;                // their refined reciprocals, valid if z_fast
    bool z_fast;                     // all three inside the division window of raster_math.h
};

// (u, v) of the integer pixel (X, Y) in projected triangle S: barycentrics, then the Affine or the
// Perspective statement.  The three points of a pixel divide by the same per-triangle numbers, so the
// quotients go through raster_math.h's shortcut (2): the refined reciprocal of a divisor is formed once
// and each quotient is the five-operation tail of the compiler's own expansion of `/`, which rounds
// identically inside the window; anything outside it (a zero barycentric on an edge, a NaN) takes `/`.
template <bool PERSPECTIVE>
CR_DEV void uv_at(const TriSetup &S, const CornerUV &k, int X, int Y, float &tu, float &tv)
{
    float n1, n2, n3, b1, b2, b3;
    numerators(S, X, Y, n1, n2, n3);
    quotients(S, n1, n2, n3, b1, b2, b3);
    if (PERSPECTIVE) {
        float q1, q2, q3;
        if (k.z_fast && in_div_window(b1) && in_div_window(b2) && in_div_window(b3)) {
            q1 = div_tail(b1, k.za, k.ra); q2 = div_tail(b2, k.zb, k.rb); q3 = div_tail(b3, k.zc, k.rc);
        } else {
            q1 = b1 / k.za; q2 = b2 / k.zb; q3 = b3 / k.zc;
        }
        const float s = (q1 + q2) + q3;
        const float nu = (k.u0 * q1 + k.u1 * q2) + k.u2 * q3, nv = (k.v0 * q1 + k.v1 * q2) + k.v2 * q3;
        if (in_div_window(s) && in_div_window(nu) && in_div_window(nv)) {
            const float r = refined_rcp(s);
            tu = div_tail(nu, s, r);
            tv = div_tail(nv, s, r);
        } else {
            tu = nu / s;
            tv = nv / s;
        }
    } else {
        tu = interp(k.u0, k.u1, k.u2, b1, b2, b3);
        tv = interp(k.v0, k.v1, k.v2, b1, b2, b3);
    }
}

}  // namespace
