// denoise_temporal_texel.hpp — the per-pixel arithmetic of idkptDenoiseTemporal's first state (the contract of include/idkpt.h, "temporal moments"): the variance of a
// pixel's mean luminance from the REPROJECTED moments (M1, M2, cnt) with the pixel's own effective sample count, a 7 x 7 guide-weighted spatial estimate where the history
// is shorter than SpatialBelow, and the demodulation of colour and variance.  The iterations that follow are denoise_variance_texel.hpp's, unchanged.  Written once for
// the device (kernels_denoise_temporal.hpp) and for a host compiler (tests/c_driver/denoise_temporal_host.cpp builds this file with g++ under ASan/UBSan).  Depends on
// <math.h> and <stdint.h> only (through denoise_variance_texel.hpp as well).  No counterpart in the reference.
//
// Every operation is a binary32 + - * / in the written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` is the IEEE division), so
// tests/denoise_temporal_ref.py restates the same text in numpy and is compared bit for bit.  No value feeds an address: a count of 0, a negative count, a NaN or an
// infinity can only make a variance that is not finite (such a pixel is left as it is by every iteration) or a weight that is NaN or zero (such a tap is dropped).
#pragma once
#include <math.h>
#include <stdint.h>
#include "denoise_variance_texel.hpp"

namespace denoisett {

using denoiset::V3;
using denoiset::v3;
using denoisevt::State;

constexpr int RADIUS = 3;                 // the spatial estimate looks at p + (dx, dy), dx and dy in -RADIUS .. RADIUS

// The spatial estimate of the variance of the mean at pixel (x, y) of a W x H image whose own guides are (ap, np) and whose effective sample count is cnt.
// fetch(qx, qy, &m, &a, &n) returns the temporal moments (M1, M2, cnt), the albedo and the normal of an IN-IMAGE texel and is never called for one outside.
// dy is the outer loop, dx the inner one; a tap outside the image is skipped.
template <class Fetch>
DENOISE_HD float spatial_variance(const Fetch& fetch, int W, int H, int x, int y, float cnt, V3 ap, V3 np, float invA, float invN)
{
    float sM1 = 0.0f, sM2 = 0.0f, sW = 0.0f;
    for (int dy = -RADIUS; dy <= RADIUS; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -RADIUS; dx <= RADIUS; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            V3 mq, aq, nq;
            fetch(qx, qy, &mq, &aq, &nq);
            const float w = 1.0f / ((1.0f + denoiset::dist2(aq, ap) * invA) * (1.0f + denoiset::dist2(nq, np) * invN));
            if (w > 0.0f && noiset::finite(mq.x) && noiset::finite(mq.y)) {      // (w > 0 is false for a NaN weight and for the zero weight of an overflowed difference)
                sM1 = sM1 + mq.x * w; sM2 = sM2 + mq.y * w;
                sW = sW + w;
            }
        }
    }
    if (sW == 0.0f) return INFINITY;
    const float a1 = sM1 / sW, a2 = sM2 / sW;
    return fmaxf(a2 - a1 * a1, 0.0f) / cnt;
}

// The state (c0, v0) the first iteration reads at pixel (x, y): t = the temporal rgb of the pixel.  invA and invN = denoiset::inv_sigma2(sigma, 0), computed once per call
// on the host.
template <class Fetch>
DENOISE_HD State temporal_state(const Fetch& fetch, int W, int H, int x, int y, V3 t, float spatialBelow, float invA, float invN, bool demod)
{
    V3 m, a, n;
    fetch(x, y, &m, &a, &n);
    const float M1 = m.x, M2 = m.y, cnt = m.z;
    State st; st.c = t;
    if (!noiset::finite(M1) || !noiset::finite(M2) || !noiset::finite(cnt)) st.v = INFINITY;
    else if (cnt >= spatialBelow) st.v = fmaxf(M2 - M1 * M1, 0.0f) / (cnt - 1.0f);
    else st.v = spatial_variance(fetch, W, H, x, y, cnt, a, n, invA, invN);
    return demod ? denoisevt::demodulate_state(st, a) : st;
}

}  // namespace denoisett
