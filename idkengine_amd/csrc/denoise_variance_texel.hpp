// denoise_variance_texel.hpp — the per-pixel arithmetic of idkptDenoiseVariance (the contract of include/idkpt.h, "variance-guided denoised output"): the variance of a
// pixel's mean luminance from the moments FinalDraw keeps (noise_texel.hpp), its demodulation, and one iteration of the a-trous filter whose luminance range kernel is
// scaled by the 3 x 3 prefiltered variance — the state (c.rgb, v) travels between the iterations, v in the alpha channel.  Written once for the device
// (kernels_denoise_variance.hpp) and for a host compiler (tests/c_driver/denoise_variance_host.cpp builds this file with g++ under ASan/UBSan).  Depends on <math.h> and
// <stdint.h> only (through denoise_texel.hpp and noise_texel.hpp as well).  No counterpart in the reference.
//
// Every operation is a binary32 + - * / in the written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` is the IEEE division), so the result
// of a pixel does not depend on where its taps come from (LDS tile or memory): tests/denoise_variance_ref.py restates the same text in numpy and is compared bit for bit.
// No value feeds an address: a NaN, an infinity or an overflowing difference can only make a WEIGHT NaN or zero, and such a tap is dropped (`w > 0`); a variance that is
// not finite takes its pixel out of every sum and leaves the pixel as it is.  One division per tap (idkptDenoise has three).
#pragma once
#include <math.h>
#include <stdint.h>
#include "denoise_texel.hpp"
#include "noise_texel.hpp"

namespace denoisevt {

using denoiset::V3;
using denoiset::v3;

struct State { V3 c; float v; };          // what an iteration reads and writes per pixel: the colour and the variance of its luminance

DENOISE_HD float lum(V3 u) { return noiset::luminance(u.x, u.y, u.z); }

// b = {1/4, 1/2, 1/4}: the 3 x 3 prefilter of the variance; every product b[i] * b[j] is exact
DENOISE_HD float prefilter_weight(int i) { return i == 1 ? 0.5f : 0.25f; }

// the variance of the pixel's MEAN luminance after n >= 2 samples; +Inf where a moment is not finite
DENOISE_HD float variance_of_mean(float m1, float m2, uint32_t n)
{
    if (!noiset::finite(m1) || !noiset::finite(m2)) return INFINITY;
    return fmaxf(m2 - m1 * m1, 0.0f) / (float)(n - 1u);
}

// a state demodulated by its pixel's own floored albedo, the variance by the square of that albedo's luminance (the end of first_state and of denoisett::temporal_state)
DENOISE_HD State demodulate_state(State st, V3 albedo)
{
    st.c = denoiset::demodulate(st.c, albedo);
    const float la = lum(v3(denoiset::albedo_floor(albedo.x), denoiset::albedo_floor(albedo.y), denoiset::albedo_floor(albedo.z)));
    st.v = st.v / (la * la);
    return st;
}
// the state the first iteration reads: (Result.rgb, v0), demodulated when `demod`
DENOISE_HD State first_state(V3 result, float m1, float m2, uint32_t n, V3 albedo, bool demod)
{
    State st; st.c = result; st.v = variance_of_mean(m1, m2, n);
    return demod ? demodulate_state(st, albedo) : st;
}

// One iteration at pixel (x, y) of a W x H image with tap spacing s.  fetch(qx, qy, &st, &a, &n) returns the state of the previous iteration (first_state for the first),
// the albedo and the normal of an IN-IMAGE texel, fetch.variance(qx, qy) its variance alone; neither is called for a texel outside.  The prefilter runs at spacing 1
// whatever s is (ey the outer loop, ex the inner one), the taps at spacing s (dy the outer loop, dx the inner one); a tap outside the image is skipped.
// ls2 = LumaSigma * LumaSigma, invA and invN = denoiset::inv_sigma2(sigma, 0): computed once per call on the host.
template <class Fetch>
DENOISE_HD State atrous_variance_texel(const Fetch& fetch, int W, int H, int x, int y, int s, float ls2, float eps, float invA, float invN)
{
    State p; V3 ap, np;
    fetch(x, y, &p, &ap, &np);
    if (!noiset::finite(p.v)) return p;
    float sumGV = 0.0f, sumG = 0.0f;
    for (int ey = -1; ey <= 1; ey++) {
        const int qy = y + ey;
        if (qy < 0 || qy >= H) continue;
        for (int ex = -1; ex <= 1; ex++) {
            const int qx = x + ex;
            if (qx < 0 || qx >= W) continue;
            const float vq = fetch.variance(qx, qy);
            if (!noiset::finite(vq)) continue;
            const float gw = prefilter_weight(ex + 1) * prefilter_weight(ey + 1);
            sumGV = sumGV + gw * vq; sumG = sumG + gw;
        }
    }
    const float g = sumGV / sumG;               // (the centre tap is in: sumG >= 1/4)
    const float invL = 1.0f / (ls2 * g + eps);
    const float lp = lum(p.c);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sumV = 0.0f, sumW = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= W) continue;
            State q; V3 aq, nq;
            fetch(qx, qy, &q, &aq, &nq);
            const float h = denoiset::kernel_weight(dx + 2) * denoiset::kernel_weight(dy + 2);
            const float dl = lum(q.c) - lp;
            const float den = ((1.0f + (dl * dl) * invL) * (1.0f + denoiset::dist2(aq, ap) * invA)) * (1.0f + denoiset::dist2(nq, np) * invN);
            const float w = h / den;
            if (w > 0.0f && noiset::finite(q.v)) {      // (w > 0 is false for a NaN weight and for the zero weight of an overflowed difference)
                sx = sx + q.c.x * w; sy = sy + q.c.y * w; sz = sz + q.c.z * w;
                sumV = sumV + q.v * (w * w);
                sumW = sumW + w;
            }
        }
    }
    if (sumW == 0.0f) return p;
    State r; r.c = v3(sx / sumW, sy / sumW, sz / sumW); r.v = sumV / (sumW * sumW);
    return r;
}

}  // namespace denoisevt
