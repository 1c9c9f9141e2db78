// kernels_present.hpp — the display image (idkptPresent; host side: host_readback.hpp): Shaders/TonemapAndGammaCorrect/compute.glsl, the one pass between
// PathTracer.Result and the swapchain (TonemapAndGammaCorrect.Compute, Source/Application.cs:217-223), on the device.  Part of the single translation unit idkpt.hip.
//
// k_present restates the shader's main, AgX_DS, DualSection, LinearToSrgb and Dither operation for operation in binary32, as kernels_sky.hpp restates the atmosphere:
//  * idkpt.hip is compiled with -ffp-contract=off: no product and sum below is fused; every operation rounds once, as written.  `/` is the IEEE division; exp and pow are
//    expf and powf, no fast-math intrinsic.
//  * What GLSL leaves to the implementation is fixed here as tests/present_ref.py fixes it: M * v sums M[0][r] v.x + M[1][r] v.y + M[2][r] v.z left to right (mat3 is
//    column-major, m[c][r]), dot sums left to right, mix(x, y, a) = x * (1 - a) + y * a, inverse(mat3) = cofactors divided by the determinant.  A GL driver may choose
//    otherwise (and its exp / pow differ), so the kernel is held to a bound measured against the binary64 value of the formula (tests/test_present_ref.py,
//    profiles/present.md), not compared bit for bit.
//  * Everything of AgX_DS that depends on the settings alone — sRGB_to_adjusted, its inverse, pow(2, exposure) — is computed once per idkptPresent by present_setup below
//    (host code of this translation unit: the same binary32 sequence, PrimariesToMatrix / ComputeCompressionMatrix / the products literally, with the shader's column-major
//    constructors and its written order sRGB_to_XYZ * XYZ_to_adjusted) and reaches the kernel by value: scalar registers, no table in memory.
//  * Sampler0-2 are sampled at texel centres of textures of the image's own size: a texel fetch.  The sum is the shader's ((0 + s0) + s1) + s2; a NULL image adds the
//    + 0.0 an unbound GL texture does.
//  * Dither: BayerMatrix8[x % 8][y % 8] — the x index FIRST, as the shader writes it —, entries k / 65.0 rounded once, (entry - 0.5) / 64.  k is computed, not looked up
//    (bayer_k below; checked against the shader's table at compile time).  y is the row of the WHOLE frame: a context that holds a shard of the rows (idkptSetRowBands,
//    idkptSetRowRange, members of a multi-device context) maps its local row to the image row first.
// Quantisation (the contract of include/idkpt.h): byte = (uint8) rintf(fminf(fmaxf(x, 0), 1) * 255.0f), alpha 255; IDKPT_DISPLAY_RGBA32F holds (dithered.rgb, 1.0).
// Thread shape: one thread per four horizontally adjacent pixels of a row — four 16-B loads, one 16-B store of four RGBA8 texels, so a wave writes 1 KB of contiguous
// bytes per row; the last W mod 4 pixels of a row are stored texel by texel.  Rows of a width that is no multiple of 4 start at 4-byte multiples only: the 16-B store
// goes through a 4-byte-aligned vector type.  The RGBA32F format stores four float4.  No LDS, no scratch.
//
// k_present_scaled: the same pass when the presentation size differs from the render size (idkptSetPresentationSize; Application.SetResolutions sizes TonemapAndGamma with
// the presentation resolution, PathTracer with the render resolution).  One invocation per PRESENTATION texel, as the shader's dispatch: uv = (texel + 0.5) / presentation
// size per axis in binary32, Sampler0 = texture(Result, uv) through the linear, clamp-to-edge filter — bloomt::sample_linear (bloom_texel.hpp), the one filter of the display
// chain, with a float4 fetch — BEFORE AgX, sRGB and dither; Sampler1 / Sampler2 have the presentation size (a texel fetch, as above); the dither is indexed by the
// presentation texel.  Same thread shape and stores.  At scales <= 1 the four texels of a thread and its neighbours share taps: the source is read about once through L1 / L2.
#pragma once
#include "bloom_texel.hpp"

namespace presentk {

struct Mat3 { float m[3][3]; };                    // column-major like GLSL: m[c][r]
struct Params {
    Mat3 toAdjusted, fromAdjusted;                 // sRGB_to_adjusted, inverse(sRGB_to_adjusted)
    float exposure2, saturation, linear, peak;     // pow(2.0, Exposure), Saturation, Linear, Peak
    int doTonemap;                                 // DoTonemapAndSrgbTransform
    int W, rows, rowMod, rowRem, bandLog2;         // the context's rows: local row -> image row as local_rows() deals them (host_context.hpp)
};

// ---- host: what depends on the settings alone (AgX_DS, compute.glsl:139-150)
static inline Mat3 inverse3(const Mat3& a)
{
#define A_(r, c) a.m[c][r]
    const float det = A_(0, 0) * (A_(1, 1) * A_(2, 2) - A_(1, 2) * A_(2, 1)) - A_(0, 1) * (A_(1, 0) * A_(2, 2) - A_(1, 2) * A_(2, 0)) + A_(0, 2) * (A_(1, 0) * A_(2, 1) - A_(1, 1) * A_(2, 0));
    Mat3 i;
    i.m[0][0] = (A_(1, 1) * A_(2, 2) - A_(1, 2) * A_(2, 1)) / det; i.m[1][0] = (A_(0, 2) * A_(2, 1) - A_(0, 1) * A_(2, 2)) / det; i.m[2][0] = (A_(0, 1) * A_(1, 2) - A_(0, 2) * A_(1, 1)) / det;
    i.m[0][1] = (A_(1, 2) * A_(2, 0) - A_(1, 0) * A_(2, 2)) / det; i.m[1][1] = (A_(0, 0) * A_(2, 2) - A_(0, 2) * A_(2, 0)) / det; i.m[2][1] = (A_(0, 2) * A_(1, 0) - A_(0, 0) * A_(1, 2)) / det;
    i.m[0][2] = (A_(1, 0) * A_(2, 1) - A_(1, 1) * A_(2, 0)) / det; i.m[1][2] = (A_(0, 1) * A_(2, 0) - A_(0, 0) * A_(2, 1)) / det; i.m[2][2] = (A_(0, 0) * A_(1, 1) - A_(0, 1) * A_(1, 0)) / det;
#undef A_
    return i;
}
static inline void mul_mv(const Mat3& a, const float v[3], float out[3]) { for (int r = 0; r < 3; r++) out[r] = a.m[0][r] * v[0] + a.m[1][r] * v[1] + a.m[2][r] * v[2]; }
static inline Mat3 mul_mm(const Mat3& a, const Mat3& b) { Mat3 o; for (int c = 0; c < 3; c++) for (int r = 0; r < 3; r++) o.m[c][r] = a.m[0][r] * b.m[c][0] + a.m[1][r] * b.m[c][1] + a.m[2][r] * b.m[c][2]; return o; }
// Unproject = xyYToXYZ(vec3(xy, 1))
static inline void unproject(const float xy[2], float out[3]) { const float Y = 1.0f; out[0] = (xy[0] * Y) / xy[1]; out[1] = Y; out[2] = ((1.0f - xy[0] - xy[1]) * Y) / xy[1]; }
static inline Mat3 primaries_to_matrix(const float r[2], const float g[2], const float b[2], const float w[2])
{
    float R[3], G[3], B[3], Wh[3], scale[3];
    unproject(r, R); unproject(g, G); unproject(b, B); unproject(w, Wh);
    const Mat3 temp = {{{R[0], 1.0f, R[2]}, {G[0], 1.0f, G[2]}, {B[0], 1.0f, B[2]}}};
    mul_mv(inverse3(temp), Wh, scale);
    Mat3 o;
    for (int i = 0; i < 3; i++) { o.m[0][i] = R[i] * scale[0]; o.m[1][i] = G[i] * scale[1]; o.m[2][i] = B[i] * scale[2]; }
    return o;
}
static inline float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
static inline void present_setup(float exposure, float compression, Params* p)
{
    const float xyR[2] = {0.64f, 0.33f}, xyG[2] = {0.3f, 0.6f}, xyB[2] = {0.15f, 0.06f}, xyW[2] = {0.3127f, 0.3290f};
    const Mat3 sRGB_to_XYZ = primaries_to_matrix(xyR, xyG, xyB, xyW);
    const float scale_factor = 1.0f / (1.0f - compression);
    const float Rc[2] = {mixf(xyW[0], xyR[0], scale_factor), mixf(xyW[1], xyR[1], scale_factor)}, Gc[2] = {mixf(xyW[0], xyG[0], scale_factor), mixf(xyW[1], xyG[1], scale_factor)},
                Bc[2] = {mixf(xyW[0], xyB[0], scale_factor), mixf(xyW[1], xyB[1], scale_factor)};
    const Mat3 adjusted_to_XYZ = primaries_to_matrix(Rc, Gc, Bc, xyW);
    p->toAdjusted = mul_mm(sRGB_to_XYZ, inverse3(adjusted_to_XYZ));
    p->fromAdjusted = inverse3(p->toAdjusted);
    p->exposure2 = powf(2.0f, exposure);
}

// ---- device
// The numerator k of BayerMatrix8[i][j] = k / 65.0 (compute.glsl:172-182).  The table is the recursive 2 x 2 pattern {{0, 3}, {2, 1}}: bit 0 of (i, j) selects the
// 16s, bit 1 the 4s, bit 2 the units; cell (a, b) of the pattern has high bit a ^ b and low bit b.
__host__ __device__ constexpr int bayer_cell(int a, int b) { return ((a ^ b) << 1) | b; }
__host__ __device__ constexpr int bayer_k(int i, int j) { return 1 + 16 * bayer_cell(i & 1, j & 1) + 4 * bayer_cell((i >> 1) & 1, (j >> 1) & 1) + bayer_cell((i >> 2) & 1, (j >> 2) & 1); }
constexpr bool bayer_matches_the_shader()
{
    constexpr int T[8][8] = {{1, 49, 13, 61, 4, 52, 16, 64}, {33, 17, 45, 29, 36, 20, 48, 32}, {9, 57, 5, 53, 12, 60, 8, 56}, {41, 25, 37, 21, 44, 28, 40, 24},
                             {3, 51, 15, 63, 2, 50, 14, 62}, {35, 19, 47, 31, 34, 18, 46, 30}, {11, 59, 7, 55, 10, 58, 6, 54}, {43, 27, 39, 23, 42, 26, 38, 22}};
    for (int i = 0; i < 8; i++) for (int j = 0; j < 8; j++) if (bayer_k(i, j) != T[i][j]) return false;
    return true;
}
static_assert(bayer_matches_the_shader(), "bayer_k must reproduce Dither's BayerMatrix8");

DEV f3 mul_mv(const Mat3& a, f3 v) { return mk3(a.m[0][0] * v.x + a.m[1][0] * v.y + a.m[2][0] * v.z, a.m[0][1] * v.x + a.m[1][1] * v.y + a.m[2][1] * v.z, a.m[0][2] * v.x + a.m[1][2] * v.y + a.m[2][2] * v.z); }
// compute.glsl:113-123
DEV float DualSection(float x, float linear, float peak)
{
    const float S = peak * linear;
    if (x < S) return x;
    const float C = peak / (peak - S);
    return peak - (peak - S) * expf((-C * (x - S)) / peak);
}
// compute.glsl:135-163 with the settings-only part precomputed
DEV f3 AgX_DS(f3 c, const Params& p)
{
    f3 w = mk3(gmax(c.x, 0.0f) * p.exposure2, gmax(c.y, 0.0f) * p.exposure2, gmax(c.z, 0.0f) * p.exposure2);
    w = mul_mv(p.toAdjusted, w);
    w = mk3(gclamp(DualSection(w.x, p.linear, p.peak), 0.0f, 1.0f), gclamp(DualSection(w.y, p.linear, p.peak), 0.0f, 1.0f), gclamp(DualSection(w.z, p.linear, p.peak), 0.0f, 1.0f));
    const float des = w.x * 0.2126729f + w.y * 0.7151522f + w.z * 0.0721750f;
    const float a = p.saturation, ia = 1.0f - a;
    w = mk3(gclamp(des * ia + w.x * a, 0.0f, 1.0f), gclamp(des * ia + w.y * a, 0.0f, 1.0f), gclamp(des * ia + w.z * a, 0.0f, 1.0f));
    return mul_mv(p.fromAdjusted, w);
}
// compute.glsl:60-67
DEV float LinearToSrgb(float v) { return v < 0.0031308f ? v * 12.92f : 1.055f * powf(v, 1.0f / 2.4f) - 0.055f; }

// main() for one texel: hdr = ((0 + s0) + s1) + s2 -> vec4(ditherdColor, 1.0)
DEV float4 present_texel(f3 hdr, int x, int y, const Params& p)
{
    f3 c;
    if (p.doTonemap) { c = AgX_DS(hdr, p); c = mk3(LinearToSrgb(c.x), LinearToSrgb(c.y), LinearToSrgb(c.z)); }
    else c = mk3(gclamp(hdr.x, 0.0f, 1.0f), gclamp(hdr.y, 0.0f, 1.0f), gclamp(hdr.z, 0.0f, 1.0f));
    const float ditherVal = ((float)bayer_k(x & 7, y & 7) / 65.0f - 0.5f) / 64.0f;
    return make_float4(c.x + ditherVal, c.y + ditherVal, c.z + ditherVal, 1.0f);
}
DEV uint32_t quantise(float4 v)
{
    const uint32_t r = (uint32_t)rintf(gmin(gmax(v.x, 0.0f), 1.0f) * 255.0f), g = (uint32_t)rintf(gmin(gmax(v.y, 0.0f), 1.0f) * 255.0f), b = (uint32_t)rintf(gmin(gmax(v.z, 0.0f), 1.0f) * 255.0f);
    return r | (g << 8) | (b << 16) | 0xff000000u;
}
// ((0 + a) + s1[i]) + s2[i]: the shader's sum once Sampler0's value a is known
DEV f3 sum_samplers(f3 a, const float4* s1, const float4* s2, size_t i)
{
    f3 h = mk3(0.0f + a.x, 0.0f + a.y, 0.0f + a.z);
    if (s1) { const float4 b = s1[i]; h = mk3(h.x + b.x, h.y + b.y, h.z + b.z); } else h = mk3(h.x + 0.0f, h.y + 0.0f, h.z + 0.0f);
    if (s2) { const float4 b = s2[i]; h = mk3(h.x + b.x, h.y + b.y, h.z + b.z); } else h = mk3(h.x + 0.0f, h.y + 0.0f, h.z + 0.0f);
    return h;
}
DEV f3 fetch_sum(const float4* s0, const float4* s1, const float4* s2, size_t i)
{
    const float4 a = s0[i];
    return sum_samplers(mk3(a.x, a.y, a.z), s1, s2, i);
}
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // four RGBA8 texels of a row that starts at any texel of the buffer
// four RGBA8 texels (n == 4: one 16-byte store) or the n < 4 of a row's tail, or n float4
template <bool F32>
DEV void store_texels(void* out, size_t base, const float4 v[4], int n)
{
    if (F32) {
        float4* o = (float4*)out + base;
#pragma unroll
        for (int k = 0; k < 4; k++) if (k < n) o[k] = v[k];
    } else {
        uint32_t* o = (uint32_t*)out + base;
        if (n == 4) { u32x4_a4 q; q.x = quantise(v[0]); q.y = quantise(v[1]); q.z = quantise(v[2]); q.w = quantise(v[3]); *(u32x4_a4*)o = q; }
        else {
#pragma unroll
            for (int k = 0; k < 3; k++) if (k < n) o[k] = quantise(v[k]);
        }
    }
}


}  // namespace presentk

// F32: IDKPT_DISPLAY_RGBA32F (out = float4 per texel) instead of RGBA8 (out = one word per texel).  Thread t: row t / quads, pixels 4 (t % quads) ... + 3 of it.
template <bool F32>
__global__ __launch_bounds__(256) void k_present(const float4* __restrict__ s0, const float4* __restrict__ s1, const float4* __restrict__ s2, void* __restrict__ out, presentk::Params p)
{
    using namespace presentk;
    const uint32_t quads = ((uint32_t)p.W + 3u) >> 2;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= quads * (uint32_t)p.rows) return;
    const int ly = (int)(t / quads), x0 = (int)(t - (uint32_t)ly * quads) * 4;
    // the image row of local row ly: a strip (rowMod 1) starts at rowRem; bands of 2^bandLog2 rows are dealt round robin (band b of this context = image band b * rowMod + rowRem)
    const int y = p.rowMod == 1 ? p.rowRem + ly : (((((ly >> p.bandLog2) * p.rowMod + p.rowRem) << p.bandLog2)) | (ly & ((1 << p.bandLog2) - 1)));
    const size_t base = (size_t)ly * (size_t)p.W + (size_t)x0;
    const int n = min(4, p.W - x0);
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < n) v[k] = present_texel(fetch_sum(s0, s1, s2, base + k), x0 + k, y, p);
    store_texels<F32>(out, base, v, n);
}

// Thread t: row t / quads of the presentation image (p.W x p.rows texels), texels 4 (t % quads) ... + 3 of it.  s0 is the W x H image of the render size; s1 / s2 have the presentation size.
template <bool F32>
__global__ __launch_bounds__(256) void k_present_scaled(const float4* __restrict__ s0, int W, int H, const float4* __restrict__ s1, const float4* __restrict__ s2, void* __restrict__ out, presentk::Params p)
{
    using namespace presentk;
    const uint32_t quads = ((uint32_t)p.W + 3u) >> 2;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= quads * (uint32_t)p.rows) return;
    const int y = (int)(t / quads), x0 = (int)(t - (uint32_t)y * quads) * 4;
    const size_t base = (size_t)y * (size_t)p.W + (size_t)x0;
    const int n = min(4, p.W - x0);
    const bloomk::DevFloatImage src = {s0, W, H};
    const float v_ = bloomt::texel_coord(y, p.rows);
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) if (k < n) {
        const bloomt::V3 a = bloomt::sample_linear(src, bloomt::texel_coord(x0 + k, p.W), v_, W, H, 0, 0);
        v[k] = present_texel(sum_samplers(mk3(a.x, a.y, a.z), s1, s2, base + k), x0 + k, y, p);
    }
    store_texels<F32>(out, base, v, n);
}
