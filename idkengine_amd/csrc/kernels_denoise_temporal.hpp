// kernels_denoise_temporal.hpp — idkptDenoiseTemporal's pre-pass (host side: host_denoise_temporal.hpp): the state (c0, v0) of include/idkpt.h ("temporal moments") that the
// iterations of kernels_denoise_variance.hpp then read with first = 0.  No counterpart in the reference; part of the single translation unit idkpt.hip.
//
// The arithmetic of one written pixel lives in denoise_temporal_texel.hpp (host- and device-clean; a host build of it is compared with tests/denoise_temporal_ref.py bit
// for bit).  k_temporal_state only decides which thread computes which pixel and where the 49 taps of the spatial estimate come from — the shape of k_denoise_var_tile<S>, on kernels_denoise.hpp's stage_tile:
// a workgroup writes a 16 x 16 tile and first stages the (16 + 6)^2 texels of temporal moments, albedo and normal its taps can touch in LDS as three float4 planes with a
// row pitch of 32 texels (33 KB).  A staged texel outside the image is left unwritten and never read (the texel function skips by the IMAGE bounds).  The temporal rgb
// is read by its own pixel alone and goes from memory straight into the stored state.  Only pixels whose count is below SpatialBelow walk the 49 taps; the others cost a
// streaming pass of 64 B in, 16 B out per pixel.
#pragma once
#include "denoise_temporal_texel.hpp"
#include "kernels_denoise.hpp"

namespace denoisetk {

using denoisek::TILE;
using denoisek::PITCH;
using denoisek::rgb;

constexpr int T = TILE + 2 * denoisett::RADIUS;      // texels per side of the staged tile

struct Params {
    int W, H;
    float spatialBelow, invA, invN;   // SpatialBelow, denoiset::inv_sigma2 of the guides' sigmas
    int demod;                        // DemodulateAlbedo
};

struct LdsFetch {                 // the staged tile: texel (x, y) of the image is slot (x - ox, y - oy); moments as (M1, M2, cnt)
    const float4* m; const float4* a; const float4* n; int ox, oy;
    __device__ inline void operator()(int x, int y, denoiset::V3* om, denoiset::V3* oa, denoiset::V3* on) const
    {
        const int k = denoisek::lds_slot(x, y, ox, oy, T);
        const float4 q = m[k];
        *om = denoiset::v3(q.x, q.y, q.w); *oa = rgb(a[k]); *on = rgb(n[k]);
    }
};

}  // namespace denoisetk

// dst = (c0.rgb, v0)
__global__ __launch_bounds__(256) void k_temporal_state(const float4* __restrict__ temporal, const float4* __restrict__ moments, const float4* __restrict__ albedo, const float4* __restrict__ normal, float4* __restrict__ dst, denoisetk::Params p)
{
    using namespace denoisetk;
    __shared__ float4 tm[T * PITCH], ta[T * PITCH], tn[T * PITCH];
    const int ox = (int)blockIdx.x * TILE - denoisett::RADIUS, oy = (int)blockIdx.y * TILE - denoisett::RADIUS;
    denoisek::stage_tile<T>(p.W, p.H, ox, oy, [&](size_t i, int k) { tm[k] = moments[i]; ta[k] = albedo[i]; tn[k] = normal[i]; });
    __syncthreads();
    int x, y; if (!denoisek::tile_pixel(p.W, p.H, &x, &y)) return;
    const LdsFetch f = {tm, ta, tn, ox, oy};
    const size_t i = (size_t)y * (size_t)p.W + (size_t)x;
    const denoisevt::State st = denoisett::temporal_state(f, p.W, p.H, x, y, rgb(temporal[i]), p.spatialBelow, p.invA, p.invN, p.demod != 0);
    dst[i] = make_float4(st.c.x, st.c.y, st.c.z, st.v);
}
