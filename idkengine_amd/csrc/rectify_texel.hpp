// rectify_texel.hpp — the per-pixel arithmetic of idkptRectifyHistory (the contract of include/idkpt.h, "history rectification"): the mean disagreement of the fast and
// the long history over the (2R + 1)^2 texels of the same surface around a pixel, its squared ratio to its own standard error, and the blend of the long history towards
// the fast one that follows from it.  Written once for the device (kernels_rectify.hpp) and for a host compiler (tests/c_driver/rectify_host.cpp builds this file with
// g++ under ASan/UBSan).  Depends on <math.h>, <stdint.h> and <string.h> only (through reproject_texel.hpp, whose V4, finite and bits_of it uses).  No counterpart in the
// reference.
//
// Every operation is a binary32 + - * / in the written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` is the IEEE division; fminf / fmaxf
// ignore a NaN operand), so tests/rectify_ref.py restates the same text in numpy and is compared bit for bit.  No value feeds an address: a NaN, an infinity or a
// difference that overflowed only drops its tap, or leaves the pixel as it is.
#pragma once
#include <math.h>
#include <stdint.h>
#include "reproject_texel.hpp"

namespace rectt {

using reprojt::V4;
using reprojt::v4;
using reprojt::finite;
using reprojt::bits_of;

constexpr int MAX_RADIUS = 3;
constexpr float MIN_TAPS = 4.0f;          // fewer contributing taps: the pixel is left as it is

struct Params {
    int W, H;
    float eps2, lo2, span;                // Epsilon * Epsilon, ZLow * ZLow, ZHigh * ZHigh - lo2: computed once per call on the host in binary32
};

struct Texel { V4 out; bool blended; };   // blended: the blend branch ran (the temporal moments' count follows out.w there)

// the difference record of a texel: (f.rgb - t.rgb, the id bits of its geometry record) — what the kernel stages and the taps read
REPROJECT_HD V4 difference(V4 f, V4 t, float idBits) { return v4(f.x - t.x, f.y - t.y, f.z - t.z, idBits); }

// One channel's squared ratio of the mean difference to its standard error
REPROJECT_HD float z2_of(float s1, float s2, float cnt, float eps2)
{
    const float m = s1 / cnt;
    const float var = fmaxf(s2 / cnt - m * m, 0.0f);
    const float se2 = var / (cnt - 1.0f);
    return (m * m) / (se2 + eps2);
}

// Pixel (x, y) of a W x H image.  fetch(qx, qy) returns the difference record of an IN-IMAGE texel and is never called for one outside; fp, tp: the pixel's own texels
// of the fast and of the long history.  dy is the outer loop, dx the inner one.
template <int R, class Fetch>
REPROJECT_HD Texel rectify_texel(const Fetch& fetch, const Params& p, int x, int y, V4 fp, V4 tp)
{
    static_assert(R >= 1 && R <= MAX_RADIUS, "the window is 3 x 3, 5 x 5 or 7 x 7");
    Texel r; r.out = tp; r.blended = false;
    const uint32_t id = bits_of(fetch(x, y).w);
    float cnt = 0.0f, s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f;
    for (int dy = -R; dy <= R; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= p.H) continue;
        for (int dx = -R; dx <= R; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= p.W) continue;
            const V4 d = fetch(qx, qy);
            if (bits_of(d.w) != id || !finite(d.x) || !finite(d.y) || !finite(d.z)) continue;
            cnt = cnt + 1.0f;
            s1x = s1x + d.x; s1y = s1y + d.y; s1z = s1z + d.z;
            s2x = s2x + d.x * d.x; s2y = s2y + d.y * d.y; s2z = s2z + d.z * d.z;
        }
    }
    if (cnt < MIN_TAPS) return r;
    const float z2 = fmaxf(fmaxf(z2_of(s1x, s2x, cnt, p.eps2), z2_of(s1y, s2y, cnt, p.eps2)), z2_of(s1z, s2z, cnt, p.eps2));
    const float lambda = fminf(fmaxf((z2 - p.lo2) / p.span, 0.0f), 1.0f);
    if (!(lambda > 0.0f)) return r;
    if (!finite(fp.x) || !finite(fp.y) || !finite(fp.z) || !finite(fp.w) || !finite(tp.x) || !finite(tp.y) || !finite(tp.z) || !finite(tp.w)) return r;
    r.out = v4(tp.x + (fp.x - tp.x) * lambda, tp.y + (fp.y - tp.y) * lambda, tp.z + (fp.z - tp.z) * lambda, tp.w + (fp.w - tp.w) * lambda);
    r.blended = true;
    return r;
}

}  // namespace rectt
