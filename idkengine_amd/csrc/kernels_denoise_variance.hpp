// kernels_denoise_variance.hpp — idkptDenoiseVariance (host side: host_denoise_variance.hpp): the variance-guided a-trous filter of include/idkpt.h, one iteration per
// launch.  No counterpart in the reference; part of the single translation unit idkpt.hip.
//
// The arithmetic of one written pixel lives in denoise_variance_texel.hpp (host- and device-clean; a host build of it is compared with tests/denoise_variance_ref.py bit
// for bit).  The kernels below only decide which thread computes which pixel and where its 25 taps and the 9 variances of the prefilter come from — the shape of
// kernels_denoise.hpp, whose tile_pixel, stage_tile and lds_slot they use:
//  * k_denoise_var_tile<S> (tap spacing S = 1, 2, 4): a workgroup writes a 16 x 16 tile and first stages the (16 + 4 S)^2 texels its taps can touch in LDS as three float4
//    planes with a row pitch of 32 texels; the variance rides in the colour plane's .w, so the footprint is k_denoise_tile<S>'s (30, 36, 48 KB).  The prefilter reads
//    p +- 1, inside the halo because 2 S >= 2.  A staged texel outside the image is left unwritten and never read (the texel function skips by the IMAGE bounds).
//  * k_denoise_var_direct (any spacing; the host uses it from spacing 8 on): the same texel function through fetches from memory.
// The first iteration is always S = 1, so making the state — Result and moments read, v0 computed, both demodulated — is fused into the tiled kernel's staging loop and the
// direct kernel never sees the moments.  Remodulation and the alpha of 1.0 are fused into the last iteration's store; every other iteration stores (c.rgb, v).
#pragma once
#include "denoise_variance_texel.hpp"
#include "kernels_denoise.hpp"

namespace denoisevk {

using denoisek::TILE;
using denoisek::PITCH;
using denoisek::rgb;

struct Params {
    int W, H, s;                  // image size, tap spacing
    float ls2, eps, invA, invN;   // LumaSigma * LumaSigma, VarianceEpsilon, denoiset::inv_sigma2 of the guides' sigmas
    uint32_t n;                   // the slot's accumulated sample count (the first iteration's v0)
    int first, last, demod;       // first / last iteration, DemodulateAlbedo
};

__device__ inline denoisevt::State state_of(float4 q) { denoisevt::State st; st.c = rgb(q); st.v = q.w; return st; }

struct MemFetch {                 // state, albedo, normal from memory: three 16-byte loads per texel
    const float4* c; const float4* a; const float4* n; int W;
    __device__ inline void operator()(int x, int y, denoisevt::State* os, denoiset::V3* oa, denoiset::V3* on) const
    {
        const size_t i = (size_t)y * (size_t)W + (size_t)x;
        *os = state_of(c[i]); *oa = rgb(a[i]); *on = rgb(n[i]);
    }
    __device__ inline float variance(int x, int y) const { return c[(size_t)y * (size_t)W + (size_t)x].w; }
};
struct LdsFetch {                 // the staged tile: texel (x, y) of the image is slot (x - ox, y - oy)
    const float4* c; const float4* a; const float4* n; int ox, oy, size;
    __device__ inline int slot(int x, int y) const { return denoisek::lds_slot(x, y, ox, oy, size); }
    __device__ inline void operator()(int x, int y, denoisevt::State* os, denoiset::V3* oa, denoiset::V3* on) const
    {
        const int k = slot(x, y);
        *os = state_of(c[k]); *oa = rgb(a[k]); *on = rgb(n[k]);
    }
    __device__ inline float variance(int x, int y) const { return c[slot(x, y)].w; }
};

__device__ inline void store_pixel(float4* __restrict__ dst, const float4* __restrict__ albedo, const Params& p, int x, int y, denoisevt::State r)
{
    const size_t i = (size_t)y * (size_t)p.W + (size_t)x;
    if (p.last) {
        if (p.demod) r.c = denoiset::remodulate(r.c, rgb(albedo[i]));
        r.v = 1.0f;
    }
    dst[i] = make_float4(r.c.x, r.c.y, r.c.z, r.v);
}

}  // namespace denoisevk

// `state` is Result when p.first (then `moments` is read as well; S == 1), else the previous iteration's (c.rgb, v) image.
template <int S>
__global__ __launch_bounds__(256) void k_denoise_var_tile(const float4* __restrict__ state, const float4* __restrict__ moments, const float4* __restrict__ albedo, const float4* __restrict__ normal, float4* __restrict__ dst, denoisevk::Params p)
{
    using namespace denoisevk;
    constexpr int T = TILE + 4 * S;
    __shared__ float4 tc[T * PITCH], ta[T * PITCH], tn[T * PITCH];
    const int ox = (int)blockIdx.x * TILE - 2 * S, oy = (int)blockIdx.y * TILE - 2 * S;
    denoisek::stage_tile<T>(p.W, p.H, ox, oy, [&](size_t i, int k) {
        float4 c = state[i]; const float4 a = albedo[i];
        if (S == 1 && p.first) {
            const float4 m = moments[i];
            const denoisevt::State st = denoisevt::first_state(rgb(c), m.x, m.y, p.n, rgb(a), p.demod != 0);
            c = make_float4(st.c.x, st.c.y, st.c.z, st.v);
        }
        tc[k] = c; ta[k] = a; tn[k] = normal[i];
    });
    __syncthreads();
    int x, y; if (!denoisek::tile_pixel(p.W, p.H, &x, &y)) return;
    const LdsFetch f = {tc, ta, tn, ox, oy, T};
    store_pixel(dst, albedo, p, x, y, denoisevt::atrous_variance_texel(f, p.W, p.H, x, y, S, p.ls2, p.eps, p.invA, p.invN));
}

// the same grid and thread mapping without the staged tile: every tap is three fetches from memory, every variance of the prefilter one.  Never the first iteration.
__global__ __launch_bounds__(256) void k_denoise_var_direct(const float4* __restrict__ state, const float4* __restrict__ albedo, const float4* __restrict__ normal, float4* __restrict__ dst, denoisevk::Params p)
{
    using namespace denoisevk;
    int x, y; if (!denoisek::tile_pixel(p.W, p.H, &x, &y)) return;
    const MemFetch f = {state, albedo, normal, p.W};
    store_pixel(dst, albedo, p, x, y, denoisevt::atrous_variance_texel(f, p.W, p.H, x, y, p.s, p.ls2, p.eps, p.invA, p.invN));
}
