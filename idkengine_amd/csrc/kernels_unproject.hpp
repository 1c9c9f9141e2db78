// kernels_unproject.hpp — an equirectangular panorama unprojected into the sky's resident faces (idkptUnprojectSky; host side: host_scene.hpp): what
// SkyBoxManager.LoadSkyBoxEquirectangular (Source/Render/SkyBoxManager.cs:115-146) does with Shaders/UnprojectEquirectangular/compute.glsl.  Part of the single translation
// unit idkpt.hip.
//
// The arithmetic of one texel and both float -> half rules live in unproject_texel.hpp (host- and device-clean; a host build of it is compared with tests/unproject_ref.py).
// The kernels below only decide which thread computes which texel:
//  * k_equirect_pack<CH>: the staged float panorama (CH = 3 or 4 floats per texel, rows as the host passed them) -> the RGBA16F image Upload2D leaves in the reference's 2-D
//    texture, 8 bytes per texel.  CH = 4: one texel per thread, one 16-byte load, one 8-byte store.  CH = 3: FOUR texels per thread — 48 contiguous bytes are three whole
//    float4 loads, the four packed texels two 16-byte stores; the last (texels % 4) texels of the image are read and written one float at a time by the thread that owns
//    them.  The staged image starts at a 256-byte boundary, so every vector access is aligned.
//  * k_sky_unproject: one thread per cube texel over 6 S^2, face-major then row then column — the resident order of DScene::sky —, four 8-byte taps of the packed panorama
//    (wrapped indices: always inside the image), one 16-byte store; consecutive threads write consecutive float4: a wave stores 1 KB of contiguous bytes.  No LDS.
#pragma once
#include "unproject_texel.hpp"

namespace unprojk {

DEV uint2 pack2(unprojt::H4 h) { return make_uint2((uint32_t)h.x | ((uint32_t)h.y << 16), (uint32_t)h.z | ((uint32_t)h.w << 16)); }

struct DevHalfImage {             // the packed panorama, one 8-byte load per texel
    const uint2* p; int w;
    DEV unprojt::H4 operator()(int x, int y) const
    {
        const uint2 q = p[(size_t)y * (size_t)w + (size_t)x];
        unprojt::H4 h; h.x = (uint16_t)(q.x & 0xffffu); h.y = (uint16_t)(q.x >> 16); h.z = (uint16_t)(q.y & 0xffffu); h.w = (uint16_t)(q.y >> 16); return h;
    }
};

}  // namespace unprojk

// texels = width * height (<= 2^27); grid ceil(texels / 256) for CH = 4, ceil(ceil(texels / 4) / 256) for CH = 3
template <int CH>
__global__ __launch_bounds__(256) void k_equirect_pack(const float* __restrict__ src, uint2* __restrict__ dst, uint32_t texels)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (CH == 4) {
        if (t >= texels) return;
        const float4 v = reinterpret_cast<const float4*>(src)[t];
        dst[t] = unprojk::pack2(unprojt::pack_texel(v.x, v.y, v.z, v.w));
    } else {
        const uint32_t first = t * 4u;                                   // (t < 2^25: no overflow)
        if (first >= texels) return;
        if (first + 4u <= texels) {
            const float4* s = reinterpret_cast<const float4*>(src) + (size_t)t * 3;
            const float4 a = s[0], b = s[1], c = s[2];
            const uint2 p0 = unprojk::pack2(unprojt::pack_texel(a.x, a.y, a.z, 1.0f)), p1 = unprojk::pack2(unprojt::pack_texel(a.w, b.x, b.y, 1.0f));
            const uint2 p2 = unprojk::pack2(unprojt::pack_texel(b.z, b.w, c.x, 1.0f)), p3 = unprojk::pack2(unprojt::pack_texel(c.y, c.z, c.w, 1.0f));
            uint4* d = reinterpret_cast<uint4*>(dst) + (size_t)t * 2;
            d[0] = make_uint4(p0.x, p0.y, p1.x, p1.y); d[1] = make_uint4(p2.x, p2.y, p3.x, p3.y);
        } else {
            for (uint32_t k = first; k < texels; k++) { const float* s = src + (size_t)k * 3; dst[k] = unprojk::pack2(unprojt::pack_texel(s[0], s[1], s[2], 1.0f)); }
        }
    }
}

// compute.glsl:13-24 for texel i of 6 S^2; pano: W x H packed texels
__global__ __launch_bounds__(256) void k_sky_unproject(const uint2* __restrict__ pano, int W, int H, float4* __restrict__ sky, int S)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t perFace = (uint32_t)S * (uint32_t)S;
    if (i >= 6u * perFace) return;
    const int face = (int)(i / perFace);
    const uint32_t t = i - (uint32_t)face * perFace;
    const int y = (int)(t / (uint32_t)S), x = (int)(t - (uint32_t)y * (uint32_t)S);
    const unprojk::DevHalfImage img = {pano, W};
    const unprojt::V4 r = unprojt::expand_half(unprojt::store_texel(unprojt::unproject_value(img, W, H, x, y, face, S)));
    sky[i] = make_float4(r.x, r.y, r.z, r.w);
}
