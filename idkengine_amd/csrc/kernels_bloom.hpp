// kernels_bloom.hpp — bloom (idkptBloom; host side: host_bloom.hpp): Shaders/Bloom/compute.glsl driven as Source/Render/Bloom.cs:56-147 drives it, the pass
// Application.cs:217-223 runs between PathTracer.Result and TonemapAndGamma.Compute.  Part of the single translation unit idkpt.hip.
//
// The arithmetic of one written texel lives in bloom_texel.hpp (host- and device-clean; a host build of it is compared with tests/bloom_ref.py bit for bit), the
// float -> half rule with it.  The kernels below only decide which thread computes which texel and where its source texels come from:
//  * k_bloom_down0: down pass 0, the one pass that reads the full-size RGBA32F image — 13 bilinear taps, 52 16-byte texels over a 6 x 6 footprint per output.  A
//    workgroup writes a 16 x 16 tile of level 0 and stages the source texels its taps can touch in LDS first.  The tile's texel range comes from the SAME binary32
//    expressions the taps evaluate (texel_coord, sample_pos: both monotone in the texel index and the offset), for the tile's first texel with offset -2 and its last
//    with offset +2; slot k of a tile row holds source texel clamp(lo + k): indices are clamped when the tile is FILLED, so a tap reads slot (unclamped index - lo)
//    and gets exactly the texel a clamped fetch from memory returns, at image edges and for odd sizes.  16 outputs span at most (16 - 1) * W / w0 + 7 <= 38 texels
//    (W <= 2 w0 + 1), so 40 x 40 slots (25.6 KB) hold every tile; the host checks the spans of a size before the first launch (host_bloom.hpp) and a slot index is
//    clamped into the tile besides.  With a presentation size (idkptSetPresentationSize) the image keeps the RENDER size while level 0 is half the PRESENTATION size:
//    uv still comes from the written level, so the same kernel reads the smaller image (render <= presentation, the engine's range: the spans only shrink).
//  * k_bloom_down0_direct: the same pass for a render size so much LARGER than the presentation size that a tile's taps span more than 40 texels (supersampling):
//    the same down_texel through a clamped fetch from memory, one 16-byte load per tap texel.  The host selects it when bloom_tile_spans_fit says no.
//  * k_bloom_pass<MODE>: every other pass, from RGBA16F levels (8-byte texel loads): MODE 0 = Downsample of down level l - 1 (with Prefilter for l = 1: the
//    reference uploads Lod = 0 for that pass too, and the shader prefilters `if (Lod == 0)`), MODE 1 = Upsample of the up (first up
//    pass: the down) level l + 1 plus one tap of down level l + 1.  The levels are a quarter of the frame and smaller: they stay in L2.
//  * k_bloom_expand: what the tonemap shader's texture(Sampler1, uv) reads, for every pixel of the frame — up level 0 magnified bilinearly — as an RGBA32F image
//    (rgb, 1.0): idkptPresent's dAdd0.  One thread per pixel, a wave writes 1 KB of contiguous bytes.  W x H is the PRESENTATION size (the size of the tonemap
//    shader's ImgResult), which is the render size unless idkptSetPresentationSize said otherwise.
// One launch per pass on the context's stream; a pass reads only what earlier launches wrote (no level is produced and consumed inside one launch).
#pragma once
#include "bloom_texel.hpp"

namespace bloomk {

constexpr int TILE = 16;          // a workgroup writes TILE x TILE texels
constexpr int SRC_TILE = 40;      // source texels staged per axis by k_bloom_down0

// the source-texel range [lo, hi] the taps of written texels [first, last] of an axis can touch (unclamped indices)
BLOOM_HD void tap_range(int first, int last, int dsize, int ssize, int reach, int* lo, int* hi)
{
    *lo = (int)floorf(bloomt::sample_pos(bloomt::texel_coord(first, dsize), ssize, -reach));
    *hi = (int)floorf(bloomt::sample_pos(bloomt::texel_coord(last, dsize), ssize, reach)) + 1;
}

struct LdsTile {                  // the staged tile of k_bloom_down0
    const float4* t; int lox, loy;
    DEV bloomt::V3 operator()(int x, int y) const
    {
        const int ix = min(max(x - lox, 0), SRC_TILE - 1), iy = min(max(y - loy, 0), SRC_TILE - 1);
        const float4 q = t[iy * SRC_TILE + ix];
        return bloomt::v3(q.x, q.y, q.z);
    }
};
struct DevHalfLevel {             // an RGBA16F level in memory, one 8-byte load per texel
    const uint2* p; int w, h;
    DEV bloomt::V3 operator()(int x, int y) const
    {
        x = min(max(x, 0), w - 1); y = min(max(y, 0), h - 1);
        const uint2 q = p[(size_t)y * (size_t)w + (size_t)x];
        return bloomt::v3(bloomt::f16_to_f32((uint16_t)(q.x & 0xffffu)), bloomt::f16_to_f32((uint16_t)(q.x >> 16)), bloomt::f16_to_f32((uint16_t)(q.y & 0xffffu)));
    }
};
struct DevFloatImage {            // an RGBA32F image in memory (the path tracer's result), one 16-byte load per texel
    const float4* p; int w, h;
    DEV bloomt::V3 operator()(int x, int y) const
    {
        x = min(max(x, 0), w - 1); y = min(max(y, 0), h - 1);
        const float4 q = p[(size_t)y * (size_t)w + (size_t)x];
        return bloomt::v3(q.x, q.y, q.z);
    }
};
// imageStore(ImgResult, imgCoord, vec4(result, 1.0)) to an RGBA16F level
DEV uint2 pack_half4(bloomt::V3 v)
{
    return make_uint2((uint32_t)bloomt::f32_to_f16_rtz(v.x) | ((uint32_t)bloomt::f32_to_f16_rtz(v.y) << 16), (uint32_t)bloomt::f32_to_f16_rtz(v.z) | (0x3C00u << 16));
}

}  // namespace bloomk

// grid (ceil(dw / 16), ceil(dh / 16)), 256 threads: thread t writes texel (16 bx + t % 16, 16 by + t / 16) of down level 0 (dw x dh) from the W x H image src
__global__ __launch_bounds__(256) void k_bloom_down0(const float4* __restrict__ src, int W, int H, uint2* __restrict__ dst, int dw, int dh, float maxColor, float threshold)
{
    using namespace bloomk;
    __shared__ float4 tile[SRC_TILE * SRC_TILE];
    const int tid = (int)threadIdx.x, tx0 = (int)blockIdx.x * TILE, ty0 = (int)blockIdx.y * TILE;
    int lox, hix, loy, hiy;
    tap_range(tx0, min(tx0 + TILE - 1, dw - 1), dw, W, 2, &lox, &hix);
    tap_range(ty0, min(ty0 + TILE - 1, dh - 1), dh, H, 2, &loy, &hiy);
    const int sx = min(hix - lox + 1, SRC_TILE), sy = min(hiy - loy + 1, SRC_TILE);
    for (int k = tid; k < sx * sy; k += 256) {
        const int ty = k / sx, tx = k - ty * sx;
        const int gx = min(max(lox + tx, 0), W - 1), gy = min(max(loy + ty, 0), H - 1);
        tile[ty * SRC_TILE + tx] = src[(size_t)gy * (size_t)W + (size_t)gx];
    }
    __syncthreads();
    const int x = tx0 + (tid & (TILE - 1)), y = ty0 + (tid >> 4);
    if (x >= dw || y >= dh) return;
    const LdsTile f = {tile, lox, loy};
    dst[(size_t)y * (size_t)dw + (size_t)x] = pack_half4(bloomt::down_texel(f, W, H, x, y, dw, dh, true, maxColor, threshold));
}

// the same pass without the staged tile (grid and thread mapping of k_bloom_pass): every tap texel is a clamped fetch from memory
__global__ __launch_bounds__(256) void k_bloom_down0_direct(const float4* __restrict__ src, int W, int H, uint2* __restrict__ dst, int dw, int dh, float maxColor, float threshold)
{
    using namespace bloomk;
    const int x = (int)blockIdx.x * TILE + ((int)threadIdx.x & (TILE - 1)), y = (int)blockIdx.y * TILE + ((int)threadIdx.x >> 4);
    if (x >= dw || y >= dh) return;
    const DevFloatImage f = {src, W, H};
    dst[(size_t)y * (size_t)dw + (size_t)x] = pack_half4(bloomt::down_texel(f, W, H, x, y, dw, dh, true, maxColor, threshold));
}

// grid (ceil(dw / 16), ceil(dh / 16)), 256 threads.  MODE 0: dst = Downsample(a), prefiltered when lodIsZero; MODE 1: dst = Upsample(a) + tap(b).  a and b are levels of sw x sh texels.
template <int MODE>
__global__ __launch_bounds__(256) void k_bloom_pass(const uint2* __restrict__ a, const uint2* __restrict__ b, int sw, int sh, uint2* __restrict__ dst, int dw, int dh, int lodIsZero, float maxColor, float threshold)
{
    using namespace bloomk;
    const int x = (int)blockIdx.x * TILE + ((int)threadIdx.x & (TILE - 1)), y = (int)blockIdx.y * TILE + ((int)threadIdx.x >> 4);
    if (x >= dw || y >= dh) return;
    const DevHalfLevel fa = {a, sw, sh};
    bloomt::V3 r;
    if (MODE == 0) r = bloomt::down_texel(fa, sw, sh, x, y, dw, dh, lodIsZero != 0, maxColor, threshold);
    else { const DevHalfLevel fb = {b, sw, sh}; r = bloomt::up_texel(fa, fb, sw, sh, x, y, dw, dh); }
    dst[(size_t)y * (size_t)dw + (size_t)x] = pack_half4(r);
}

// grid ceil(W * H / 256), 256 threads: pixel i = y * W + x of the frame
__global__ __launch_bounds__(256) void k_bloom_expand(const uint2* __restrict__ up0, int sw, int sh, float4* __restrict__ out, int W, int H)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)W * (size_t)H) return;
    const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * (size_t)W);
    const bloomk::DevHalfLevel f = {up0, sw, sh};
    const bloomt::V3 r = bloomt::expand_texel(f, sw, sh, x, y, W, H);
    out[i] = make_float4(r.x, r.y, r.z, 1.0f);
}
