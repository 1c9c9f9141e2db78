// kernels_reconstruct.hpp — idkptReconstructHistory (host side: host_reconstruct.hpp), the contract of include/idkpt.h ("history reconstruction").  No counterpart in
// the reference; part of the single translation unit idkpt.hip.
//
// The arithmetic of one pixel lives in reconstruct_texel.hpp (host- and device-clean; a host build of it is compared with tests/reconstruct_ref.py bit for bit).
// k_reconstruct<R> only decides which thread computes which pixel: 16 x 16 pixel tiles through kernels_denoise.hpp's tile_pixel, one thread per pixel, every fetch
// from memory.  No LDS: only the pixels whose count is below FillBelow walk taps, and those are sparse; the far taps of Stride > 1 would need a halo of up to 24 texels
// around a tile of 16.  A thread reads its own temporal texel and the .w of its geometry record first (20 B) and leaves before anything else is fetched when the pixel
// keeps its bits; a filled pixel reads its guides, up to (2R + 1)^2 - 1 taps of 20 B, the guides (32 B) of those that passed the history tests, and stores 16 B.
//
// IN PLACE: `t` is read and written.  A written pixel has a count below FillBelow; a tap contributes only with a count of at least FillBelow; the count (.w) is stored
// with the bits it had.  So a thread that reads a texel another thread is writing drops it by its count, whichever of the two rgb values it saw, and no result depends
// on the order in which workgroups run.  No spare image, no swap.  (`t` is therefore neither const nor __restrict__.)
//
// Resources (hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage), R = 1 / 2 / 3: 45 / 47 / 39 VGPRs, 36 / 38 / 38 SGPRs, 0 B scratch,
// 0 B LDS, 8 waves per SIMD; no atomics, no per-lane arrays (four scalar accumulators).  Times and what the call gives: profiles/reconstruct.md.
#pragma once
#include "reconstruct_texel.hpp"
#include "kernels_denoise.hpp"

namespace reconk {

struct MemFetch {                 // every texel from memory; only asked for in-image positions (reconstruct_texel tests the tap first)
    const float4* t; const float4* g; const float4* a; const float4* n; int W;
    __device__ inline size_t at(int x, int y) const { return (size_t)y * (size_t)W + (size_t)x; }
    __device__ inline void history(int x, int y, recont::V4* ot, uint32_t* oid) const
    {
        const size_t i = at(x, y);
        const float4 q = t[i];
        *ot = recont::v4(q.x, q.y, q.z, q.w); *oid = __float_as_uint(g[i].w);
    }
    __device__ inline void guides(int x, int y, denoiset::V3* oa, denoiset::V3* on) const
    {
        const size_t i = at(x, y);
        *oa = denoisek::rgb(a[i]); *on = denoisek::rgb(n[i]);
    }
};

}  // namespace reconk

// grid (ceil(W / 16), ceil(H / 16)), 256 threads.  t: the slot's temporal image (read and written); g: its geometry image; a, n: its accumulated Albedo and Normal
template <int R>
__global__ __launch_bounds__(256) void k_reconstruct(float4* t, const float4* __restrict__ g, const float4* __restrict__ a, const float4* __restrict__ n, recont::Params p)
{
    int x, y; if (!denoisek::tile_pixel(p.W, p.H, &x, &y)) return;
    const reconk::MemFetch fetch = {t, g, a, n, p.W};
    const recont::Texel r = recont::reconstruct_texel<R>(fetch, p, x, y);
    if (r.written) t[(size_t)y * (size_t)p.W + (size_t)x] = make_float4(r.out.x, r.out.y, r.out.z, r.out.w);
}
