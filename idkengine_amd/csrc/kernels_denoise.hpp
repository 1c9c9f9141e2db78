// kernels_denoise.hpp — idkptDenoise (host side: host_denoise.hpp): the edge-avoiding a-trous filter of include/idkpt.h, one iteration per launch.  No counterpart in the
// reference (its denoiser is OIDN on the host); part of the single translation unit idkpt.hip.
//
// The arithmetic of one written pixel lives in denoise_texel.hpp (host- and device-clean; a host build of it is compared with tests/denoise_ref.py bit for bit).  The
// kernels below only decide which thread computes which pixel and where its 25 taps come from.  A pixel reads 25 x 48 bytes (colour, albedo, normal) and writes 16; the
// compulsory traffic is 48 + 16 bytes, so the work is in the staging:
//  * k_denoise_tile<S> (tap spacing S = 1, 2, 4): a workgroup writes a 16 x 16 tile and first stages the (16 + 4 S)^2 texels its taps can touch — 20^2, 24^2, 32^2 — in LDS
//    as three float4 planes with a row pitch of 32 texels (a ds_read_b128's 16-lane groups then fall on distinct slots): 30, 36 and 48 KB.  A staged texel outside the
//    image is left unwritten and never read (atrous_texel skips the tap by the IMAGE bounds, the same test on both routes).
//  * k_denoise_direct (any spacing; the host uses it from spacing 8 on, where the halo would be 4x the tile and more): the same atrous_texel through fetches from memory.
// Demodulation is fused into the first iteration (every colour it reads is divided by its own pixel's floored albedo: the staged copy on the tiled route, per fetch on the
// direct one — the same operation on the same operands either way), remodulation into the last one's store.  The stored alpha is 1.0.
#pragma once
#include "denoise_texel.hpp"

namespace denoisek {

constexpr int TILE = 16;          // a workgroup writes TILE x TILE pixels
constexpr int PITCH = 32;         // texels per staged row (>= 16 + 4 * 4)
constexpr int MAX_TILE_SPACING = 4;

struct Params {
    int W, H, s;                  // image size, tap spacing
    float invC, invA, invN;       // denoiset::inv_sigma2 of the three sigmas, the colour's for this iteration
    int demodIn, remodOut;        // first / last iteration with DemodulateAlbedo
};

__device__ inline denoiset::V3 rgb(float4 q) { return denoiset::v3(q.x, q.y, q.z); }

struct MemFetch {                 // colour, albedo, normal from memory: three 16-byte loads per texel
    const float4* c; const float4* a; const float4* n; int W; bool demod;
    __device__ inline void operator()(int x, int y, denoiset::V3* oc, denoiset::V3* oa, denoiset::V3* on) const
    {
        const size_t i = (size_t)y * (size_t)W + (size_t)x;
        *oa = rgb(a[i]); *on = rgb(n[i]);
        const denoiset::V3 col = rgb(c[i]);
        *oc = demod ? denoiset::demodulate(col, *oa) : col;
    }
};
struct LdsFetch {                 // the staged tile: texel (x, y) of the image is slot (x - ox, y - oy)
    const float4* c; const float4* a; const float4* n; int ox, oy, size;
    __device__ inline void operator()(int x, int y, denoiset::V3* oc, denoiset::V3* oa, denoiset::V3* on) const
    {
        const int ix = min(max(x - ox, 0), size - 1), iy = min(max(y - oy, 0), size - 1), k = iy * PITCH + ix;
        *oc = rgb(c[k]); *oa = rgb(a[k]); *on = rgb(n[k]);
    }
};

__device__ inline void store_pixel(float4* __restrict__ dst, const float4* __restrict__ albedo, const Params& p, int x, int y, denoiset::V3 r)
{
    const size_t i = (size_t)y * (size_t)p.W + (size_t)x;
    if (p.remodOut) r = denoiset::remodulate(r, rgb(albedo[i]));
    dst[i] = make_float4(r.x, r.y, r.z, 1.0f);
}

}  // namespace denoisek

// grid (ceil(W / 16), ceil(H / 16)), 256 threads: thread t writes pixel (16 bx + t % 16, 16 by + t / 16)
template <int S>
__global__ __launch_bounds__(256) void k_denoise_tile(const float4* __restrict__ colour, const float4* __restrict__ albedo, const float4* __restrict__ normal, float4* __restrict__ dst, denoisek::Params p)
{
    using namespace denoisek;
    static_assert(S >= 1 && S <= MAX_TILE_SPACING && TILE + 4 * S <= PITCH, "the staged tile must fit its pitch");
    constexpr int T = TILE + 4 * S;
    __shared__ float4 tc[T * PITCH], ta[T * PITCH], tn[T * PITCH];
    const int tid = (int)threadIdx.x, ox = (int)blockIdx.x * TILE - 2 * S, oy = (int)blockIdx.y * TILE - 2 * S;
    for (int k = tid; k < T * T; k += 256) {
        const int ty = k / T, tx = k - ty * T, gx = ox + tx, gy = oy + ty;
        if (gx < 0 || gx >= p.W || gy < 0 || gy >= p.H) continue;
        const size_t i = (size_t)gy * (size_t)p.W + (size_t)gx;
        const float4 c = colour[i], a = albedo[i];
        const denoiset::V3 col = p.demodIn ? denoiset::demodulate(rgb(c), rgb(a)) : rgb(c);
        tc[ty * PITCH + tx] = make_float4(col.x, col.y, col.z, 1.0f); ta[ty * PITCH + tx] = a; tn[ty * PITCH + tx] = normal[i];
    }
    __syncthreads();
    const int x = (int)blockIdx.x * TILE + (tid & (TILE - 1)), y = (int)blockIdx.y * TILE + (tid >> 4);
    if (x >= p.W || y >= p.H) return;
    const LdsFetch f = {tc, ta, tn, ox, oy, T};
    store_pixel(dst, albedo, p, x, y, denoiset::atrous_texel(f, p.W, p.H, x, y, S, p.invC, p.invA, p.invN));
}

// the same grid and thread mapping without the staged tile: every tap is three fetches from memory
__global__ __launch_bounds__(256) void k_denoise_direct(const float4* __restrict__ colour, const float4* __restrict__ albedo, const float4* __restrict__ normal, float4* __restrict__ dst, denoisek::Params p)
{
    using namespace denoisek;
    const int x = (int)blockIdx.x * TILE + ((int)threadIdx.x & (TILE - 1)), y = (int)blockIdx.y * TILE + ((int)threadIdx.x >> 4);
    if (x >= p.W || y >= p.H) return;
    const MemFetch f = {colour, albedo, normal, p.W, p.demodIn != 0};
    store_pixel(dst, albedo, p, x, y, denoiset::atrous_texel(f, p.W, p.H, x, y, p.s, p.invC, p.invA, p.invN));
}
