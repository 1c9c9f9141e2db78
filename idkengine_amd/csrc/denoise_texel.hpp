// denoise_texel.hpp — the per-pixel arithmetic of idkptDenoise (the contract of include/idkpt.h, "denoised output"): one iteration of the edge-avoiding a-trous wavelet
// filter (Dammertz et al. 2010) with RATIONAL (Cauchy) range kernels, albedo demodulation and the sigma schedule.  Written once for the device (kernels_denoise.hpp)
// and for a host compiler (tests/c_driver/denoise_host.cpp builds this file with g++ under ASan/UBSan).  Depends on <math.h> and <stdint.h> only.
//
// Every operation is a binary32 + - * / in the written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` is the IEEE division), so the result
// of a pixel does not depend on where its taps come from (LDS tile or memory): tests/denoise_ref.py restates the same text in numpy and is compared bit for bit.
// No texel value feeds an address: a NaN, an infinity or an overflowing difference can only make a WEIGHT NaN or zero, and such a tap is dropped (`w > 0`).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DENOISE_HD __host__ __device__ inline
#else
#define DENOISE_HD inline
#endif

namespace denoiset {

struct V3 { float x, y, z; };
DENOISE_HD V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }

constexpr float EPS = 1e-3f;              // the floor of the albedo in de- and remodulation
constexpr int MAX_ITERATIONS = 8;

// k = {1/16, 1/4, 3/8, 1/4, 1/16}: the B3 spline; every product k[i] * k[j] is exact
DENOISE_HD float kernel_weight(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }

// 1 / (sigma_i * sigma_i) with sigma_i = sigma * 2^-i (the colour sigma halves every iteration; the guides' sigmas use i = 0); computed once per launch, on the host
DENOISE_HD float inv_sigma2(float sigma, int i) { const float s = ldexpf(sigma, -i); return 1.0f / (s * s); }

// fmaxf semantics: a NaN albedo channel acts as EPS
DENOISE_HD float albedo_floor(float a) { return fmaxf(a, EPS); }
DENOISE_HD V3 demodulate(V3 c, V3 a) { return v3(c.x / albedo_floor(a.x), c.y / albedo_floor(a.y), c.z / albedo_floor(a.z)); }
DENOISE_HD V3 remodulate(V3 c, V3 a) { return v3(c.x * albedo_floor(a.x), c.y * albedo_floor(a.y), c.z * albedo_floor(a.z)); }

// |u_q - u_p|^2, summed left to right
DENOISE_HD float dist2(V3 q, V3 p)
{
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// One iteration at pixel (x, y) of a W x H image with tap spacing s.  fetch(qx, qy, &c, &a, &n) returns the colour of the previous iteration (the demodulated result for
// the first), the albedo and the normal of an IN-IMAGE texel; it is never called for a texel outside.  dy is the outer loop, dx the inner one; a tap outside is skipped.
template <class Fetch>
DENOISE_HD V3 atrous_texel(const Fetch& fetch, int W, int H, int x, int y, int s, float invC, float invA, float invN)
{
    V3 cp, ap, np;
    fetch(x, y, &cp, &ap, &np);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sumW = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= W) continue;
            V3 cq, aq, nq;
            fetch(qx, qy, &cq, &aq, &nq);
            const float h = kernel_weight(dx + 2) * kernel_weight(dy + 2);
            const float w = ((h * (1.0f / (1.0f + dist2(cq, cp) * invC))) * (1.0f / (1.0f + dist2(aq, ap) * invA))) * (1.0f / (1.0f + dist2(nq, np) * invN));
            if (w > 0.0f) {                     // (false for a NaN weight and for the zero weight of an overflowed difference)
                sx = sx + cq.x * w; sy = sy + cq.y * w; sz = sz + cq.z * w;
                sumW = sumW + w;
            }
        }
    }
    if (sumW == 0.0f) return cp;
    return v3(sx / sumW, sy / sumW, sz / sumW);
}

}  // namespace denoiset
