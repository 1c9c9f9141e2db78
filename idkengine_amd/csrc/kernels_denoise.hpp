// kernels_denoise.hpp — idkptDenoise (host side: host_denoise.hpp): the edge-avoiding a-trous filter of include/idkpt.h, one iteration per launch.  No counterpart in the
// reference (its denoiser is OIDN on the host); part of the single translation unit idkpt.hip.
//
// The arithmetic of one written pixel lives in denoise_texel.hpp (host- and device-clean; a host build of it is compared with tests/denoise_ref.py bit for bit).  The
// kernels below only decide which thread computes which pixel and where its 25 taps come from; the pixel mapping, the staging loop and the clamp of a staged slot
// (tile_pixel, stage_tile, lds_slot) are stated here once for the three filters.  A pixel reads 25 x 48 bytes (colour, albedo, normal) and writes 16; the
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

// ---- what the kernels of the three filters share (kernels_denoise_variance.hpp, kernels_denoise_temporal.hpp): grid (ceil(W / 16), ceil(H / 16)), 256 threads
// the pixel thread t writes, (16 bx + t % 16, 16 by + t / 16); false where the image has no such pixel
__device__ inline bool tile_pixel(int W, int H, int* x, int* y) { *x = (int)blockIdx.x * TILE + ((int)threadIdx.x & (TILE - 1)); *y = (int)blockIdx.y * TILE + ((int)threadIdx.x >> 4); return *x < W && *y < H; }
// The staging loop over the T x T texels from (ox, oy) on, the tile and its halo: put(i, k) does the kernel's loads and stores for each one inside the image, i its index
// in the image, k its slot in a plane of PITCH texels per row.  A texel outside the image is left unwritten.  The kernel's __syncthreads() follows the call.
template <int T, class Put>
__device__ inline void stage_tile(int W, int H, int ox, int oy, const Put& put)
{
    static_assert(T > TILE && T <= PITCH, "the staged tile must fit its pitch");
    for (int k = (int)threadIdx.x; k < T * T; k += 256) {
        const int ty = k / T, tx = k - ty * T, gx = ox + tx, gy = oy + ty;
        if (gx < 0 || gx >= W || gy < 0 || gy >= H) continue;
        put((size_t)gy * (size_t)W + (size_t)gx, ty * PITCH + tx);
    }
}
// the slot of image texel (x, y) in a staged tile of `size` texels per side whose slot 0 is texel (ox, oy); clamped: no value reaches outside the planes
__device__ inline int lds_slot(int x, int y, int ox, int oy, int size) { return min(max(y - oy, 0), size - 1) * PITCH + min(max(x - ox, 0), size - 1); }

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
        const int k = lds_slot(x, y, ox, oy, size);
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

template <int S>
__global__ __launch_bounds__(256) void k_denoise_tile(const float4* __restrict__ colour, const float4* __restrict__ albedo, const float4* __restrict__ normal, float4* __restrict__ dst, denoisek::Params p)
{
    using namespace denoisek;
    constexpr int T = TILE + 4 * S;
    __shared__ float4 tc[T * PITCH], ta[T * PITCH], tn[T * PITCH];
    const int ox = (int)blockIdx.x * TILE - 2 * S, oy = (int)blockIdx.y * TILE - 2 * S;
    stage_tile<T>(p.W, p.H, ox, oy, [&](size_t i, int k) {
        const float4 c = colour[i], a = albedo[i];
        const denoiset::V3 col = p.demodIn ? denoiset::demodulate(rgb(c), rgb(a)) : rgb(c);
        tc[k] = make_float4(col.x, col.y, col.z, 1.0f); ta[k] = a; tn[k] = normal[i];
    });
    __syncthreads();
    int x, y; if (!tile_pixel(p.W, p.H, &x, &y)) return;
    const LdsFetch f = {tc, ta, tn, ox, oy, T};
    store_pixel(dst, albedo, p, x, y, denoiset::atrous_texel(f, p.W, p.H, x, y, S, p.invC, p.invA, p.invN));
}

// the same grid and thread mapping without the staged tile: every tap is three fetches from memory
__global__ __launch_bounds__(256) void k_denoise_direct(const float4* __restrict__ colour, const float4* __restrict__ albedo, const float4* __restrict__ normal, float4* __restrict__ dst, denoisek::Params p)
{
    using namespace denoisek;
    int x, y; if (!tile_pixel(p.W, p.H, &x, &y)) return;
    const MemFetch f = {colour, albedo, normal, p.W, p.demodIn != 0};
    store_pixel(dst, albedo, p, x, y, denoiset::atrous_texel(f, p.W, p.H, x, y, p.s, p.invC, p.invA, p.invN));
}
