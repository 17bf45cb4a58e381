// mip_sample.h — what the two texture passes over a mip chain share (texmip.hip: trilinear; texaniso.hip:
// anisotropic): the chain's layout, the level of a footprint, and (u, v) of a pixel and of its two neighbours through
// raster_math.h's TriSetup.  The block constant, host_f32_to_i32, texel and bilinear are not here: every pass over
// the winner plane needs them, so they are winner_pass.h's.  Each translation unit gets its own copy (anonymous
// namespace); include after common.h, crender_mip.h and winner_pass.h.
#pragma once

namespace {

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

// The chain of a th x tw texture for a kernel's arguments; false for a texture crender_mip_layout refuses.
inline bool mip_chain(int th, int tw, MipChain &M)
{
    int h[kMaxLevels], w[kMaxLevels];
    unsigned long long total;
    M.th = th;
    M.tw = tw;
    return chain_layout(th, tw, M.L, h, w, M.off, total);
}

// The lower level l0 and the weight f of the one above it for a footprint of rho texels, of a chain of L levels.
CR_DEV void mip_level(float rho, int L, int &l0, float &f)
{
    l0 = 0;
    f = 0.0f;
    if (rho > 1.0f) {
        if (!(rho < (float)(1u << (L - 1)))) {
            l0 = L - 1;
        } else {
            // 1 < rho < 2^15: a normal number whose exponent field is the level, and whose
            // significand, scaled back by the exact power of two, is 1 + f
            l0 = (int)(__float_as_uint(rho) >> 23) - 127;
            f = rho * __uint_as_float((uint32_t)(127 - l0) << 23) - 1.0f;
        }
    }
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

// (u, v) of a covered pixel and of its right and lower neighbours: the winner projected once, one TriSetup for the three.
struct PixelUV {
    float tu, tv, ux, vx, uy, vy;
};

template <bool PERSPECTIVE>
CR_DEV PixelUV pixel_uv(const ProjConst &P, const float *__restrict__ tri, const float *__restrict__ uv,
                        const WinnerPixel &p)
{
    const float *w = uv + p.orig * 6;
    CornerUV K{w[0], w[1], w[2], w[3], w[4], w[5], 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, false};
    float raw[3][3];
    const TriXYZ X = winner_triangle(tri, p.t, P, raw);
    K.za = raw[0][2]; K.zb = raw[1][2]; K.zc = raw[2][2];
    if (PERSPECTIVE && in_div_window(K.za) && in_div_window(K.zb) && in_div_window(K.zc)) {
        K.ra = refined_rcp(K.za); K.rb = refined_rcp(K.zb); K.rc = refined_rcp(K.zc);
        K.z_fast = true;
    }
    const TriSetup S = make_setup(X, true);
    PixelUV r;
    uv_at<PERSPECTIVE>(S, K, p.x, p.y, r.tu, r.tv);
    uv_at<PERSPECTIVE>(S, K, p.x + 1, p.y, r.ux, r.vx);
    uv_at<PERSPECTIVE>(S, K, p.x, p.y + 1, r.uy, r.vy);
    return r;
}

}  // namespace
