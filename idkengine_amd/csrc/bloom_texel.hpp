// bloom_texel.hpp — the per-texel arithmetic of Shaders/Bloom/compute.glsl (main, Downsample, Upsample, Prefilter), the sizes of Source/Render/Bloom.cs:129-147 and the
// RGBA16F storage rule, written once for the device (kernels_bloom.hpp) and for a host compiler (tests/c_driver/bloom_host.cpp builds this file with g++ under
// ASan/UBSan).  Depends on <math.h>, <stddef.h> and <stdint.h> only.
//
// Every operation is binary32 in the shader's written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` is the IEEE division):
//  * uv = (imgCoord + 0.5) / imgSize of the WRITTEN level, per axis;
//  * textureLod / textureLodOffset at an explicit level with a linear filter and clamp to edge: the GL 4.6 8.14.2 arithmetic SampleTex (pt_kernels.hpp) uses —
//    f = u * size - 0.5 + offset, i0 = floor(f), weight = f - i0, texels i0 and i0 + 1 with CLAMPED INDICES, mix(mix(t00, t10, ax), mix(t01, t11, ax), ay),
//    mix(x, y, a) = x * (1 - a) + y * a;
//  * the thirteen sums of Downsample and the nine of Upsample left to right as the shader writes them, then `* 0.25` and `/ 16.0`.
// Storage (the contract of include/idkpt.h): a level is R16G16B16A16Float, alpha 1.0 (0x3C00).  float -> half ROUNDS TOWARD ZERO, a finite value beyond 65504 becomes
// 65504, subnormal halves are produced, +-Inf stays +-Inf, NaN becomes a quiet NaN (f32_to_f16_rtz below).  Mesa llvmpipe's imageStore to an RGBA16F image follows
// this rule on every texel of tests/golden/bloom/chain.npz (tests/test_bloom_ref.py).  half -> float is exact.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BLOOM_HD __host__ __device__ inline
#else
#define BLOOM_HD inline
#endif

namespace bloomt {

struct V3 { float x, y, z; };
BLOOM_HD V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
BLOOM_HD V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
BLOOM_HD V3 mul(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
BLOOM_HD V3 div(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
BLOOM_HD float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
BLOOM_HD float minf(float x, float y) { return y < x ? y : x; }      // GLSL min / max
BLOOM_HD float maxf(float x, float y) { return x < y ? y : x; }

BLOOM_HD uint32_t f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
BLOOM_HD float bits_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// ---- storage: binary32 -> binary16, round toward zero
BLOOM_HD uint16_t f32_to_f16_rtz(float f)
{
    const uint32_t u = f32_bits(f), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t)(sign | (a == 0x7f800000u ? 0x7c00u : 0x7e00u));   // Inf; NaN
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7bffu);                                  // >= 65536: saturates to 65504 ((65504, 65536) truncates to it below)
    const uint32_t e = a >> 23;
    if (e >= 113u) return (uint16_t)(sign | ((a - (112u << 23)) >> 13));                     // normal half: drop 13 mantissa bits
    if (e < 102u) return (uint16_t)sign;                                                      // below the smallest subnormal half (2^-24)
    return (uint16_t)(sign | (((a & 0x7fffffu) | 0x800000u) >> (126u - e)));                  // subnormal half: multiples of 2^-24
}
BLOOM_HD float f16_to_f32(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 0u) { const float v = (float)m * 5.9604644775390625e-8f; return bits_f32(f32_bits(v) | sign); }   // m * 2^-24, exact
    if (e == 31u) return bits_f32(sign | 0x7f800000u | (m << 13));
    return bits_f32(sign | ((e + 112u) << 23) | (m << 13));
}

// ---- sizes (Bloom.SetSize, BBG.Texture.GetMaxMipmapLevel / GetMipmapLevelSize)
BLOOM_HD int ilog2i(int v) { int l = 0; while (v > 1) { v >>= 1; l++; } return l; }
// W, H >= 2.  *w0, *h0: level 0 (integer division: floor); returns the number of levels of the down chain (the up chain has one fewer)
BLOOM_HD int bloom_levels(int W, int H, int minusLods, int* w0, int* h0)
{
    *w0 = W / 2; *h0 = H / 2;
    const int full = ilog2i(*w0 > *h0 ? *w0 : *h0) + 1;
    const int l = minusLods >= full ? 0 : full - minusLods;
    return l > 2 ? l : 2;
}
BLOOM_HD int level_dim(int d0, int level) { const int d = level < 31 ? d0 >> level : 0; return d > 1 ? d : 1; }

// ---- sampling.  Fetch: V3 operator()(int x, int y) const, called with UNCLAMPED texel indices; it returns the texel at the clamped ones.
BLOOM_HD float texel_coord(int i, int n) { return ((float)i + 0.5f) / (float)n; }                // uv of the written level's texel i
BLOOM_HD float sample_pos(float u, int size, int offset) { return u * (float)size - 0.5f + (float)offset; }
template <class Fetch>
BLOOM_HD V3 sample_linear(const Fetch& fetch, float u, float v, int w, int h, int ox, int oy)
{
    const float fx = sample_pos(u, w, ox), fy = sample_pos(v, h, oy);
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const V3 a = fetch(x0, y0), b = fetch(x0 + 1, y0), c = fetch(x0, y0 + 1), d = fetch(x0 + 1, y0 + 1);
    return v3(mixf(mixf(a.x, b.x, ax), mixf(c.x, d.x, ax), ay), mixf(mixf(a.y, b.y, ax), mixf(c.y, d.y, ax), ay), mixf(mixf(a.z, b.z, ax), mixf(c.z, d.z, ax), ay));
}
// Tap: V3 operator()(int ox, int oy) const = textureLodOffset(src, uv, lod, ivec2(ox, oy)).rgb

// compute.glsl:56-90
template <class Tap>
BLOOM_HD V3 downsample(const Tap& t)
{
    const V3 center = t(0, 0), yellowUpRight = t(0, 2), yellowDownLeft = t(-2, 0), greenDownRight = t(2, 0), blueDownLeft = t(0, -2);
    V3 yellow = t(-2, 2); yellow = add(yellow, yellowUpRight); yellow = add(yellow, center); yellow = add(yellow, yellowDownLeft);
    V3 green = yellowUpRight; green = add(green, t(2, 2)); green = add(green, greenDownRight); green = add(green, center);
    V3 blue = center; blue = add(blue, greenDownRight); blue = add(blue, t(2, -2)); blue = add(blue, blueDownLeft);
    V3 lila = yellowDownLeft; lila = add(lila, center); lila = add(lila, blueDownLeft); lila = add(lila, t(-2, -2));
    V3 red = t(-1, 1); red = add(red, t(1, 1)); red = add(red, t(1, -1)); red = add(red, t(-1, -1));
    return mul(add(mul(red, 0.5f), mul(add(add(add(yellow, green), blue), lila), 0.125f)), 0.25f);
}
// compute.glsl:92-107
template <class Tap>
BLOOM_HD V3 upsample(const Tap& t)
{
    V3 r = mul(t(-1, 1), 1.0f); r = add(r, mul(t(0, 1), 2.0f)); r = add(r, mul(t(1, 1), 1.0f));
    r = add(r, mul(t(-1, 0), 2.0f)); r = add(r, mul(t(0, 0), 4.0f)); r = add(r, mul(t(1, 0), 2.0f));
    r = add(r, mul(t(-1, -1), 1.0f)); r = add(r, mul(t(0, -1), 2.0f)); r = add(r, mul(t(1, -1), 1.0f));
    return div(r, 16.0f);
}
// compute.glsl:109-122.  Knee * 2.0 and 0.25 / Knee are binary32 operations on the binary32 constant 0.2.
BLOOM_HD V3 prefilter(V3 c, float maxColor, float threshold)
{
    const float Knee = 0.2f;
    c = v3(minf(maxColor, c.x), minf(maxColor, c.y), minf(maxColor, c.z));
    const float brightness = maxf(maxf(c.x, c.y), c.z);
    const float cx = threshold - Knee, cy = Knee * 2.0f, cz = 0.25f / Knee;
    float rq = minf(maxf(brightness - cx, 0.0f), cy);
    rq = (rq * rq) * cz;
    const float s = maxf(rq, brightness - threshold) / maxf(brightness, 0.0001f);
    return mul(c, s);
}

// ---- the four passes for one written texel (x, y) of a level of dw x dh texels; the sources are sw x sh
template <class Fetch> struct TapOf {
    const Fetch& f; float u, v; int w, h;
    BLOOM_HD V3 operator()(int ox, int oy) const { return sample_linear(f, u, v, w, h, ox, oy); }
};
// The down pass that writes level l: Downsample(src, Lod), and Prefilter `if (Lod == 0)`.  Bloom.cs uploads Lod = 0 for level 0 (src = the image) AND Lod =
// currentWriteLod - 1 = 0 for level 1 (src = down level 0): the reference prefilters twice, and so does this (lodIsZero = l <= 1); from level 2 on Lod = l - 1 > 0.
template <class Fetch>
BLOOM_HD V3 down_texel(const Fetch& src, int sw, int sh, int x, int y, int dw, int dh, bool lodIsZero, float maxColor, float threshold)
{
    const TapOf<Fetch> t = {src, texel_coord(x, dw), texel_coord(y, dh), sw, sh};
    const V3 r = downsample(t);
    return lodIsZero ? prefilter(r, maxColor, threshold) : r;
}
// up pass: Upsample(SamplerUpsample, uv, Lod) + textureLod(SamplerDownsample, uv, Lod).rgb; both levels have Lod's size sw x sh
template <class FetchUp, class FetchDown>
BLOOM_HD V3 up_texel(const FetchUp& up, const FetchDown& down, int sw, int sh, int x, int y, int dw, int dh)
{
    const float u = texel_coord(x, dw), v = texel_coord(y, dh);
    const TapOf<FetchUp> t = {up, u, v, sw, sh};
    return add(upsample(t), sample_linear(down, u, v, sw, sh, 0, 0));
}
// what the tonemap shader reads: texture(Sampler1, (p + 0.5) / imageSize) on up level 0 (sw x sh), magnified to the W x H frame
template <class Fetch>
BLOOM_HD V3 expand_texel(const Fetch& up0, int sw, int sh, int x, int y, int W, int H)
{
    return sample_linear(up0, texel_coord(x, W), texel_coord(y, H), sw, sh, 0, 0);
}

// a level of RGBA16F texels in memory (four uint16 per texel), fetched with clamped indices
struct HalfLevel {
    const uint16_t* p; int w, h;
    BLOOM_HD V3 operator()(int x, int y) const
    {
        x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x); y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
        const uint16_t* t = p + ((size_t)y * (size_t)w + (size_t)x) * 4;
        return v3(f16_to_f32(t[0]), f16_to_f32(t[1]), f16_to_f32(t[2]));
    }
};
// an RGBA32F image in memory
struct FloatImage {
    const float* p; int w, h;
    BLOOM_HD V3 operator()(int x, int y) const
    {
        x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x); y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
        const float* t = p + ((size_t)y * (size_t)w + (size_t)x) * 4;
        return v3(t[0], t[1], t[2]);
    }
};

}  // namespace bloomt
