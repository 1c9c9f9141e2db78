// kernels_rectify.hpp — idkptRectifyHistory (host side: host_rectify.hpp), the contract of include/idkpt.h ("history rectification").  No counterpart in the reference;
// part of the single translation unit idkpt.hip.
//
// The arithmetic of one written pixel lives in rectify_texel.hpp (host- and device-clean; a host build of it is compared with tests/rectify_ref.py bit for bit).
// k_rectify<R, MOMENTS> only decides which thread computes which pixel and where the (2R + 1)^2 taps come from — the shape of k_temporal_state, on kernels_denoise.hpp's
// stage_tile: a workgroup writes a 16 x 16 tile and first stages the (16 + 2R)^2 difference records (f.rgb - t.rgb, id bits) its taps can touch in LDS as ONE float4 plane
// with a row pitch of 32 texels (R = 1, 2, 3: 9, 10, 11 KB).  The difference is formed once, at staging — the same correctly rounded value wherever it is formed — so a
// tap is one ds_read_b128 instead of two.  A staged texel outside the image is left unwritten and never read (the texel function skips by the IMAGE bounds).  Only the
// pixel's own f and t come from memory again, for the blend.  Traffic per pixel: 48 B in for the staging (plus the halo's share), 32 B in and 16 B out for the own pixel,
// 4 B more where MOMENTS and the blend ran.
// Reads precede writes: `out` is another buffer than `t` (the host swaps them afterwards), so no workgroup sees a neighbour's result.
#pragma once
#include "rectify_texel.hpp"
#include "kernels_denoise.hpp"

namespace rectk {

using denoisek::TILE;
using denoisek::PITCH;

__device__ inline rectt::V4 v4_of(float4 q) { return rectt::v4(q.x, q.y, q.z, q.w); }

struct LdsFetch {                 // the staged tile: texel (x, y) of the image is slot (x - ox, y - oy)
    const float4* d; int ox, oy, size;
    __device__ inline rectt::V4 operator()(int x, int y) const { return v4_of(d[denoisek::lds_slot(x, y, ox, oy, size)]); }
};

}  // namespace rectk

// grid (ceil(W / 16), ceil(H / 16)), 256 threads.  t / f / g: the slot's temporal, fast temporal and geometry images; out: the spare image; moments: the slot's temporal
// moments image (MOMENTS only), of which the .w of a blended pixel is written and nothing is read
template <int R, bool MOMENTS>
__global__ __launch_bounds__(256) void k_rectify(const float4* __restrict__ t, const float4* __restrict__ f, const float4* __restrict__ g, float4* __restrict__ out, float4* __restrict__ moments, rectt::Params p)
{
    using namespace rectk;
    constexpr int T = TILE + 2 * R;
    __shared__ float4 td[T * PITCH];
    const int ox = (int)blockIdx.x * TILE - R, oy = (int)blockIdx.y * TILE - R;
    denoisek::stage_tile<T>(p.W, p.H, ox, oy, [&](size_t i, int k) {
        const rectt::V4 d = rectt::difference(v4_of(f[i]), v4_of(t[i]), g[i].w);
        td[k] = make_float4(d.x, d.y, d.z, d.w);
    });
    __syncthreads();
    int x, y; if (!denoisek::tile_pixel(p.W, p.H, &x, &y)) return;
    const LdsFetch fetch = {td, ox, oy, T};
    const size_t i = (size_t)y * (size_t)p.W + (size_t)x;
    const rectt::Texel r = rectt::rectify_texel<R>(fetch, p, x, y, v4_of(f[i]), v4_of(t[i]));
    out[i] = make_float4(r.out.x, r.out.y, r.out.z, r.out.w);
    if (MOMENTS && r.blended) moments[i].w = r.out.w;
}
