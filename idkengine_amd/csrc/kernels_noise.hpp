// kernels_noise.hpp — idkptEstimateNoise (host side: host_noise.hpp): the per-tile error map and its summary from a slot's moments image, the contract of include/idkpt.h
// ("noise estimate").  No counterpart in the reference (it decides "denoise now" by a fixed sample count); part of the single translation unit idkpt.hip.
//
// The arithmetic of a pixel and of a tree level lives in noise_texel.hpp (host- and device-clean; a host build of it is compared with tests/noise_ref.py bit for bit).
// The kernel only maps a tile to a wave: 8 x 8 pixels are the 64 lanes, lane j = (y & 7) * 8 + (x & 7), and level `mask` of the pairwise tree is one exchange with lane
// j ^ mask — every lane ends with the same sum.  The maximum runs over the same exchanges (e >= 0 and never NaN: any order gives the same bits).  Lane 0 writes the tile's
// two floats and the two aggregates: an atomic add of 1 and an atomic max on the bit pattern of a non-negative float, both independent of the order the tiles arrive in.
// A pixel reads 16 B, a tile writes 8: the launch is one pass over the moments.
#pragma once
#include "noise_texel.hpp"

namespace noisek {

constexpr int WAVES = 4;                                  // tiles per 256-thread block
enum { SUM_TILES_ABOVE = 0, SUM_MAX_TILE_MEAN = 1, SUM_TILES = 2, SUM_SAMPLES = 3, SUM_WORDS = 4 };   // idkpt_noise_summary, as dwords

}  // namespace noisek

// grid ceil(tiles / 4), 256 threads; `summary` was zeroed in stream order before the launch
__global__ __launch_bounds__(256) void k_noise_estimate(const float4* __restrict__ moments, int W, int H, uint32_t n, float epsilon, float threshold, float2* __restrict__ tiles, uint32_t* __restrict__ summary)
{
    using namespace noisek;
    const uint32_t tilesX = ((uint32_t)W + 7u) / 8u, tilesY = ((uint32_t)H + 7u) / 8u, nTiles = tilesX * tilesY;
    if (blockIdx.x == 0 && threadIdx.x == 0) { summary[SUM_TILES] = nTiles; summary[SUM_SAMPLES] = n; }
    const uint32_t tile = blockIdx.x * WAVES + (threadIdx.x >> 6), j = threadIdx.x & 63u;
    if (tile >= nTiles) return;                           // (the whole wave)
    const uint32_t x = (tile % tilesX) * 8u + (j & 7u), y = (tile / tilesX) * 8u + (j >> 3);
    const bool inside = x < (uint32_t)W && y < (uint32_t)H;
    float e = 0.0f;                                       // a position outside the image counts as 0
    if (inside) { const float4 m = moments[(size_t)y * (size_t)W + x]; e = noiset::pixel_error(m.x, m.y, n, epsilon); }
    const int count = (int)__popcll(__ballot(inside));    // >= 1: the tile's first pixel is inside
    float v = e, mx = e;
    for (int mask = 1; mask < noiset::TILE_TEXELS; mask <<= 1) {
        v = noiset::tree_step(v, __shfl_xor(v, mask, 64));
        mx = fmaxf(mx, __shfl_xor(mx, mask, 64));
    }
    if (j != 0u) return;
    const float mean = noiset::tile_mean(v, count);
    tiles[tile] = make_float2(mean, mx);
    if (mean > threshold) atomicAdd(&summary[SUM_TILES_ABOVE], 1u);
    atomicMax(&summary[SUM_MAX_TILE_MEAN], __float_as_uint(mean));
}
