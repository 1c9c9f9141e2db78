// noise_texel.hpp — the per-texel arithmetic of the noise estimate (the contract of include/idkpt.h, "noise estimate"): the fold of one sample's luminance into the
// moments (m1, m2) that FinalDraw keeps while idkptSetNoiseEstimate is on, the per-pixel relative standard error idkptEstimateNoise derives from them, and the steps of
// the 8 x 8 tile's pairwise sum.  Written once for the device (kernels_frame.hpp, kernels_noise.hpp) and for a host compiler (tests/c_driver/noise_host.cpp builds this
// file with g++ under ASan/UBSan).  Depends on <math.h> and <stdint.h> only.  No counterpart in the reference.
//
// Every operation is a binary32 + - * / or sqrt in the written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` and sqrtf are the correctly
// rounded forms), so tests/noise_ref.py restates the same text in numpy and is compared bit for bit.  No value feeds an address.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NOISE_HD __host__ __device__ inline
#else
#define NOISE_HD inline
#endif

namespace noiset {

constexpr int TILE = 8;                   // the first-hit stage's tile grid
constexpr int TILE_TEXELS = TILE * TILE;  // position j = (y & 7) * 8 + (x & 7)

// Rec. 709 luminance of the value FinalDraw folds into Result
NOISE_HD float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// GLSL mix, as FinalDraw's own fold (pt_device.hpp gmix): x * (1 - a) + y * a
NOISE_HD float mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }

// one sample of luminance L with FinalDraw's weight w = 1 / (accumulated + 1)
NOISE_HD void fold(float* m1, float* m2, float L, float w)
{
    *m1 = mix(*m1, L, w);
    *m2 = mix(*m2, L * L, w);
}

NOISE_HD bool finite(float v) { return v - v == 0.0f; }

// the relative standard error of the pixel's mean luminance after n >= 2 samples; +Inf where a moment is not finite
NOISE_HD float pixel_error(float m1, float m2, uint32_t n, float epsilon)
{
    if (!finite(m1) || !finite(m2)) return INFINITY;
    const float var = fmaxf(m2 - m1 * m1, 0.0f);
    return sqrtf(var / (float)(n - 1u)) / (fmaxf(m1, 0.0f) + epsilon);
}

// One level of the tile's pairwise tree: position j adds the value position j ^ mask held BEFORE the level (the sum is commutative: both partners end with the same bits).
// The levels run mask = 1, 2, 4, 8, 16, 32; after the last every position holds the tile's sum.
NOISE_HD float tree_step(float own, float partner) { return own + partner; }

// the tile's two floats from the tree's sum, the maximum and the count of pixels inside the image (>= 1)
NOISE_HD float tile_mean(float sum, int inside) { return sum / (float)inside; }

#if !defined(__HIP_DEVICE_COMPILE__)
// the whole tile on one thread (host builds): e[j] of the 64 positions, positions outside the image hold 0 and inside[j] = 0
inline void tile_reduce(const float* e, const uint8_t* inside, float* mean, float* max)
{
    float v[TILE_TEXELS], t[TILE_TEXELS], mx = 0.0f; int count = 0;
    for (int j = 0; j < TILE_TEXELS; j++) { v[j] = inside[j] ? e[j] : 0.0f; if (inside[j]) { count++; mx = fmaxf(mx, e[j]); } }
    for (int mask = 1; mask < TILE_TEXELS; mask <<= 1) {
        for (int j = 0; j < TILE_TEXELS; j++) t[j] = tree_step(v[j], v[j ^ mask]);
        for (int j = 0; j < TILE_TEXELS; j++) v[j] = t[j];
    }
    *mean = tile_mean(v[0], count); *max = mx;
}
#endif

}  // namespace noiset
