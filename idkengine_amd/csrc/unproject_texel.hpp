// unproject_texel.hpp — the per-texel arithmetic of SkyBoxManager.LoadSkyBoxEquirectangular (Source/Render/SkyBoxManager.cs:115-146): the upload of the float panorama into an
// R16G16B16A16Float texture and Shaders/UnprojectEquirectangular/compute.glsl (main, SampleSphericalMap, SrgbToLinear) into the R16G16B16A16Float cube map, written once for
// the device (kernels_unproject.hpp) and for a host compiler (tests/c_driver/unproject_host.cpp builds this file with g++ under ASan/UBSan).  Depends on bloom_texel.hpp
// (the half conversions) and <math.h> only.
//
// Upload (pack_texel): GL leaves the float -> half conversion of a pixel transfer to the driver.  Mesa llvmpipe — the rule tests/golden/unproject/cases.npz holds on every
// texel, read back as GL_HALF_FLOAT (tests/test_unproject_ref.py) — ROUNDS TO NEAREST, TIES TO EVEN, and PRODUCES SUBNORMAL HALVES (a value below 2^-25 becomes a signed
// zero); f32_to_f16_rne below.  Three channels get alpha 1.0 (0x3C00).
//   One deliberate deviation: a finite input whose nearest half would be infinite (|v| >= 65520) is stored as +-65504, never infinity.  An infinite sky texel makes every
//   sample that sees it infinite, and the store below saturates too.  (idkptUnprojectSky refuses non-finite inputs, so no Inf / NaN reaches this.)
// Shader (unproject_texel), every operation binary32 in the shader's written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` is the IEEE division):
//  * uv = (xy + 0.5) / S, ndc = uv * 2 - 1, GetWorldSpaceDirection(ndc, face) of include/Math.glsl:17-39 with normalize(v) = v * (1 / sqrt(dot(v, v))), dot summed left to
//    right (the convention of this library: pt_device.hpp, kernels_sky.hpp);
//  * SampleSphericalMap: atan2f(z, x), asinf(y), * (0.1591, 0.3183), + 0.5.  atan2f of signed zeros FOLLOWS C (Annex F): atan2f(+0, x < 0) = +pi, atan2f(-0, x < 0) = -pi,
//    atan2f(+-0, +0) = +-0.  GLSL leaves these to the driver; they occur in the centre column of face -X and at the centres of faces +Y and -Y, at odd S only;
//  * texture(SamplerEquirectangular, uv): the reference never configures this texture, so it has the GL defaults: wrap S and T REPEAT, one level, level of detail 0 in a
//    compute shader = magnification = LINEAR.  The GL 4.6 8.14.2 arithmetic SampleTex (pt_kernels.hpp) uses: f = u * size - 0.5, i0 = floor(f), weight = f - i0, texels
//    i0 and i0 + 1 WRAPPED MODULO THE SIZE (not clamped as in bloom), mix(mix(t00, t10, ax), mix(t01, t11, ax), ay), mix(x, y, a) = x * (1 - a) + y * a; all four channels;
//  * SrgbToLinear exactly as written — the reference applies it to HDR data, and so does this: c < 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f) on R, G, B
//    (a selection: a NaN of the unselected branch does not propagate), alpha unchanged;
//  * imageStore to the RGBA16F cube: f32_to_f16_rtz (bloom_texel.hpp), the rule Mesa llvmpipe's imageStore follows on every texel of this shader's fixture as well.
// The resident sky is the stored half expanded to float (exact).
#pragma once
#include "bloom_texel.hpp"

namespace unprojt {

using bloomt::f32_bits;
using bloomt::f32_to_f16_rtz;
using bloomt::f16_to_f32;
using bloomt::mixf;

struct V4 { float x, y, z, w; };
struct H4 { uint16_t x, y, z, w; };

// ---- upload: binary32 -> binary16, round to nearest even, subnormals produced, finite overflow -> 65504.  Inf / NaN as IEEE (not reached through the library).
BLOOM_HD uint16_t f32_to_f16_rne(float f)
{
    const uint32_t u = f32_bits(f), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t)(sign | (a == 0x7f800000u ? 0x7c00u : 0x7e00u));
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7bffu);                                  // >= 65520: the nearest half would be infinite -> 65504
    const uint32_t e = a >> 23;
    if (e >= 113u) {                                                                          // normal half: 13 mantissa bits are rounded away (a carry moves into the exponent)
        const uint32_t v = a - (112u << 23), r = v & 0x1fffu; uint32_t h = v >> 13;
        if (r > 0x1000u || (r == 0x1000u && (h & 1u))) h++;
        return (uint16_t)(sign | h);
    }
    if (e < 102u) return (uint16_t)sign;                                                      // < 2^-25: zero (2^-25 itself is a tie and goes to the even zero below)
    const uint32_t m = (a & 0x7fffffu) | 0x800000u, sh = 126u - e;                            // subnormal half: multiples of 2^-24; sh in 14..24
    const uint32_t half = 1u << (sh - 1u), r = m & ((1u << sh) - 1u); uint32_t h = m >> sh;
    if (r > half || (r == half && (h & 1u))) h++;
    return (uint16_t)(sign | h);
}
BLOOM_HD H4 pack_texel(float r, float g, float b, float a)
{
    H4 h; h.x = f32_to_f16_rne(r); h.y = f32_to_f16_rne(g); h.z = f32_to_f16_rne(b); h.w = f32_to_f16_rne(a); return h;
}

// ---- the shader
// include/Math.glsl:17-39 (the overload taking ndc and the face), normalised
BLOOM_HD void world_direction(float x, float y, int face, float* dx, float* dy, float* dz)
{
    float vx, vy, vz;
    switch (face) {
        case 0: vx = 1.0f; vy = -y; vz = -x; break;
        case 1: vx = -1.0f; vy = -y; vz = x; break;
        case 2: vx = x; vy = 1.0f; vz = y; break;
        case 3: vx = x; vy = -1.0f; vz = -y; break;
        case 4: vx = x; vy = -y; vz = 1.0f; break;
        default: vx = -x; vy = -y; vz = -1.0f; break;
    }
    const float inv = 1.0f / sqrtf(vx * vx + vy * vy + vz * vz);
    *dx = vx * inv; *dy = vy * inv; *dz = vz * inv;
}
BLOOM_HD float texel_ndc(int i, int S) { const float uv = ((float)i + 0.5f) / (float)S; return uv * 2.0f - 1.0f; }
// compute.glsl:26-35
BLOOM_HD void spherical_uv(float dx, float dy, float dz, float* u, float* v)
{
    *u = atan2f(dz, dx) * 0.1591f + 0.5f;
    *v = asinf(dy) * 0.3183f + 0.5f;
}
// GL_REPEAT of a texel index (|i| is far below 2^31: |u| <= 1, size <= 16384)
BLOOM_HD int wrap_repeat(int i, int n) { const int m = i % n; return m < 0 ? m + n : m; }
// the linear filter's footprint for coordinate u of an axis of `size` texels: wrapped indices and the weight of the second
BLOOM_HD void linear_taps(float u, int size, int* i0, int* i1, float* a)
{
    const float f = u * (float)size - 0.5f, f0 = floorf(f);
    *a = f - f0;
    *i0 = wrap_repeat((int)f0, size); *i1 = wrap_repeat((int)f0 + 1, size);
}
BLOOM_HD float srgb_to_linear(float c) { return c < 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f); }
BLOOM_HD V4 expand_half(H4 h) { V4 v; v.x = f16_to_f32(h.x); v.y = f16_to_f32(h.y); v.z = f16_to_f32(h.z); v.w = f16_to_f32(h.w); return v; }

// one cube texel (x, y) of face `face`: the value imageStore receives.  Fetch: H4 operator()(int x, int y) const on the packed panorama, indices already wrapped.
template <class Fetch>
BLOOM_HD V4 unproject_value(const Fetch& fetch, int W, int H, int x, int y, int face, int S)
{
    float dx, dy, dz, u, v;
    world_direction(texel_ndc(x, S), texel_ndc(y, S), face, &dx, &dy, &dz);
    spherical_uv(dx, dy, dz, &u, &v);
    int x0, x1, y0, y1; float ax, ay;
    linear_taps(u, W, &x0, &x1, &ax);
    linear_taps(v, H, &y0, &y1, &ay);
    const V4 a = expand_half(fetch(x0, y0)), b = expand_half(fetch(x1, y0)), c = expand_half(fetch(x0, y1)), d = expand_half(fetch(x1, y1));
    V4 r;
    r.x = srgb_to_linear(mixf(mixf(a.x, b.x, ax), mixf(c.x, d.x, ax), ay));
    r.y = srgb_to_linear(mixf(mixf(a.y, b.y, ax), mixf(c.y, d.y, ax), ay));
    r.z = srgb_to_linear(mixf(mixf(a.z, b.z, ax), mixf(c.z, d.z, ax), ay));
    r.w = mixf(mixf(a.w, b.w, ax), mixf(c.w, d.w, ax), ay);
    return r;
}
// ... and what the cube map holds of it, expanded: the resident texel
BLOOM_HD H4 store_texel(V4 v) { H4 h; h.x = f32_to_f16_rtz(v.x); h.y = f32_to_f16_rtz(v.y); h.z = f32_to_f16_rtz(v.z); h.w = f32_to_f16_rtz(v.w); return h; }

// the packed panorama in memory (four uint16 per texel)
struct HalfImage {
    const uint16_t* p; int w;
    BLOOM_HD H4 operator()(int x, int y) const
    {
        const uint16_t* t = p + ((size_t)y * (size_t)w + (size_t)x) * 4;
        H4 h; h.x = t[0]; h.y = t[1]; h.z = t[2]; h.w = t[3]; return h;
    }
};

}  // namespace unprojt
