// kernels_reproject.hpp — idkptCaptureGeometry, idkptReproject and idkptUseTemporalAsDenoised (host side: host_reproject.hpp), the contract of include/idkpt.h ("temporal
// reprojection").  No counterpart in the reference (it resets the accumulation on a camera move and waits); part of the single translation unit idkpt.hip.
//
// The arithmetic of a record and of a reprojected pixel lives in reproject_texel.hpp (host- and device-clean; a host build of it is compared with tests/reproject_ref.py bit
// for bit).  The kernels below only map threads to pixels:
//  * k_geom_rays writes one idkpt_ray per pixel, through the pixel centre, for the closest-hit core behind idkptTraceRaysDevice; k_geom_pack turns the rays and the core's
//    hits into the slot's geometry image.  Two streaming passes of 32 B in / 32 B out and 64 B in / 16 B out per pixel; the traversal between them dominates.
//  * k_reproject: a workgroup is a 16 x 16 pixel tile (thread t = pixel (16 bx + t % 16, 16 by + t / 16)).  A pixel reads its own Result and record (32 B, coalesced: a
//    wave covers four 256-B row segments) and gathers four neighbouring (record, temporal) pairs of the history slot at a position that moves smoothly with the pixel, so
//    the gathers of a tile fall into a tile-sized window of neighbouring lines and the four taps of neighbouring pixels share them (a 1 x 256 strip would touch four times
//    as many rows of the history images).  Compulsory traffic 32 + 32 B in, 16 B out per pixel: memory-bound.  No LDS (nothing is reused across threads that the cache does
//    not already serve), no scratch; the camera travels in the kernel arguments.
//  * k_reproject_moments (idkptReprojectMoments): the same mapping and the same gathers on the slot's luminance moments and the history slot's temporal moments image.
//  * k_temporal_to_denoised: rgb of the temporal image with alpha 1.0, the denoised image's format.
//  * k_geom_motion_pack (idkptCaptureMotion): k_geom_pack fused with the motion record of motion_texel.hpp — where the hit surface stood in the previous frame;
//    k_reproject_motion<MOMENTS>: the two reprojections of a slot that holds such a record.  Measured: profiles/motion.md.
#pragma once
#include "reproject_texel.hpp"
#include "motion_texel.hpp"

namespace reprojk {

constexpr int TILE = 16;          // a workgroup writes TILE x TILE pixels
struct Camera { float invProj[16], invView[16]; };

struct MemFetch {                 // geometry record and temporal texel of the history slot: two 16-byte loads
    const float4* g; const float4* c; int W;
    __device__ inline void operator()(int x, int y, reprojt::V4* og, reprojt::V4* oc) const
    {
        const size_t i = (size_t)y * (size_t)W + (size_t)x;
        const float4 a = g[i], b = c[i];
        *og = reprojt::v4(a.x, a.y, a.z, a.w); *oc = reprojt::v4(b.x, b.y, b.z, b.w);
    }
};

}  // namespace reprojk

// grid ceil(N / 256), 256 threads; N = W * H pixels of the whole frame, row-major
__global__ __launch_bounds__(256) void k_geom_rays(reprojk::Camera cam, int W, int H, uint32_t N, idkpt_ray* __restrict__ rays)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int x = (int)(i % (uint32_t)W), y = (int)(i / (uint32_t)W);
    const float nx = ((float)x + 0.5f) / (float)W * 2.0f - 1.0f, ny = ((float)y + 0.5f) / (float)H * 2.0f - 1.0f;   // the first-hit stage's expression before its jitter
    const f3 d = GetWorldSpaceDirection(cam.invProj, cam.invView, nx, ny);
    ((float4*)rays)[2 * (size_t)i] = make_float4(cam.invView[12], cam.invView[13], cam.invView[14], reprojt::FLOAT_MAX);
    ((float4*)rays)[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, 0.0f);
}

__global__ __launch_bounds__(256) void k_geom_pack(const idkpt_ray* __restrict__ rays, const idkpt_hit* __restrict__ hits, uint32_t N, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float4 a = ((const float4*)rays)[2 * (size_t)i], b = ((const float4*)rays)[2 * (size_t)i + 1];
    const float T = ((const float*)hits)[8 * (size_t)i];
    const uint2 h = ((const uint2*)hits)[4 * (size_t)i + 2];                  // MeshTransformId, Hit
    const float o[3] = {a.x, a.y, a.z}, d[3] = {b.x, b.y, b.z};
    const reprojt::V4 r = reprojt::pack_record(o, d, T, h.x, h.y != 0u);
    out[i] = make_float4(r.x, r.y, r.z, r.w);
}

// idkptCaptureMotion: k_geom_pack's grid and mapping; the ray and the hit are read once (64 B) and BOTH records written (2 x 16 B), all coalesced.  A hit gathers its
// triangle's indices (16 B), the three previous positions (3 x 12 B of motionPrev) and the PrevModel rows of its instance (48 B: float4 6-8 of the nine per transform, the
// convention of load_inv_model_at): primary hits of neighbouring pixels share triangles and transforms, so the caches serve the gathers.  No LDS, no scratch, no atomics.
// Every id is checked against its table before it feeds an address (motion_texel.hpp); geom is written exactly as k_geom_pack writes it.
__global__ __launch_bounds__(256) void k_geom_motion_pack(const idkpt_ray* __restrict__ rays, const idkpt_hit* __restrict__ hits, uint32_t N, const uint4* __restrict__ tris, uint32_t triCount,
                                                          const float* __restrict__ motionPrev, uint32_t vertexCount, const float4* __restrict__ xforms, uint32_t xformCount,
                                                          float4* __restrict__ geom, float4* __restrict__ motion)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float4 a = ((const float4*)rays)[2 * (size_t)i], b = ((const float4*)rays)[2 * (size_t)i + 1];
    const float4 t = ((const float4*)hits)[2 * (size_t)i];                      // T, BaryX, BaryY, TriangleId
    const uint2 h = ((const uint2*)hits)[4 * (size_t)i + 2];                  // MeshTransformId, Hit
    const float o[3] = {a.x, a.y, a.z}, d[3] = {b.x, b.y, b.z};
    const reprojt::V4 r = reprojt::pack_record(o, d, t.x, h.x, h.y != 0u);
    reprojt::V4 m = r;                                                         // a miss: the same record
    const uint32_t tri = __float_as_uint(t.w);
    if (h.y != 0u && motiont::ids_resident(tri, triCount, h.x, xformCount)) {
        const uint4 v = tris[tri];
        if (motiont::vertices_resident(v.x, v.y, v.z, vertexCount)) {
            const float* p0 = motionPrev + 3 * (size_t)v.x; const float* p1 = motionPrev + 3 * (size_t)v.y; const float* p2 = motionPrev + 3 * (size_t)v.z;
            const float q0[3] = {p0[0], p0[1], p0[2]}, q1[3] = {p1[0], p1[1], p1[2]}, q2[3] = {p2[0], p2[1], p2[2]};
            const float4* x = xforms + 9 * (size_t)h.x;
            const float4 r0 = x[6], r1 = x[7], r2 = x[8];
            m = motiont::prev_record(t.y, t.z, q0, q1, q2, reprojt::v4(r0.x, r0.y, r0.z, r0.w), reprojt::v4(r1.x, r1.y, r1.z, r1.w), reprojt::v4(r2.x, r2.y, r2.z, r2.w), h.x);
        }
    }
    geom[i] = make_float4(r.x, r.y, r.z, r.w);
    motion[i] = make_float4(m.x, m.y, m.z, m.w);
}

// grid (ceil(W / 16), ceil(H / 16)), 256 threads.  hg / hc: the history slot's images, or both null to start a history (out = (cur.rgb, n))
__global__ __launch_bounds__(256) void k_reproject(const float4* __restrict__ cur, const float4* __restrict__ g, const float4* __restrict__ hg, const float4* __restrict__ hc,
                                                   float4* __restrict__ out, reprojt::Params p)
{
    using namespace reprojk;
    const int x = (int)blockIdx.x * TILE + ((int)threadIdx.x & (TILE - 1)), y = (int)blockIdx.y * TILE + ((int)threadIdx.x >> 4);
    if (x >= p.W || y >= p.H) return;
    const size_t i = (size_t)y * (size_t)p.W + (size_t)x;
    const float4 c = cur[i];
    if (!hg) { out[i] = make_float4(c.x, c.y, c.z, p.n); return; }
    const float4 r = g[i];
    const MemFetch f = {hg, hc, p.W};
    const reprojt::V4 o = reprojt::reproject_texel(f, p, reprojt::v4(c.x, c.y, c.z, c.w), reprojt::v4(r.x, r.y, r.z, r.w));
    out[i] = make_float4(o.x, o.y, o.z, o.w);
}

// idkptReprojectMoments: k_reproject's grid, thread mapping and traffic on the luminance moments.  mom: the slot's moments image (m1, m2, 0, 1); hg / hm: the history
// slot's geometry and temporal moments images, or both null to start a history (out = (m1, m2, 0, n)).  No LDS, no scratch.
__global__ __launch_bounds__(256) void k_reproject_moments(const float4* __restrict__ mom, const float4* __restrict__ g, const float4* __restrict__ hg, const float4* __restrict__ hm,
                                                           float4* __restrict__ out, reprojt::Params p)
{
    using namespace reprojk;
    const int x = (int)blockIdx.x * TILE + ((int)threadIdx.x & (TILE - 1)), y = (int)blockIdx.y * TILE + ((int)threadIdx.x >> 4);
    if (x >= p.W || y >= p.H) return;
    const size_t i = (size_t)y * (size_t)p.W + (size_t)x;
    const float4 m = mom[i];
    if (!hg) { out[i] = make_float4(m.x, m.y, 0.0f, p.n); return; }
    const float4 r = g[i];
    const MemFetch f = {hg, hm, p.W};
    const reprojt::V4 o = reprojt::reproject_moments_texel(f, p, m.x, m.y, reprojt::v4(r.x, r.y, r.z, r.w));
    out[i] = make_float4(o.x, o.y, o.z, o.w);
}

// idkptReproject / idkptReprojectMoments of a slot that holds a MOTION image (idkptCaptureMotion) onto a history: k_reproject's / k_reproject_moments' grid, mapping and
// gathers plus one more coalesced 16-byte read per pixel — the motion record mv[i], which is looked up in the history in place of the geometry record (the lookup record of
// reproject_texel.hpp).  in: Result (MOMENTS: the moments image) of the slot; hg / hc: the history slot's geometry and temporal (MOMENTS: temporal moments) images, never null
// (a history is started by the kernels above).  No LDS, no scratch.
template <bool MOMENTS>
__global__ __launch_bounds__(256) void k_reproject_motion(const float4* __restrict__ in, const float4* __restrict__ g, const float4* __restrict__ mv, const float4* __restrict__ hg,
                                                          const float4* __restrict__ hc, float4* __restrict__ out, reprojt::Params p)
{
    using namespace reprojk;
    const int x = (int)blockIdx.x * TILE + ((int)threadIdx.x & (TILE - 1)), y = (int)blockIdx.y * TILE + ((int)threadIdx.x >> 4);
    if (x >= p.W || y >= p.H) return;
    const size_t i = (size_t)y * (size_t)p.W + (size_t)x;
    const float4 c = in[i], r = g[i], l = mv[i];
    const MemFetch f = {hg, hc, p.W};
    const reprojt::V4 rg = reprojt::v4(r.x, r.y, r.z, r.w), rl = reprojt::v4(l.x, l.y, l.z, l.w);
    const reprojt::V4 o = MOMENTS ? reprojt::reproject_moments_texel(f, p, c.x, c.y, rg, rl) : reprojt::reproject_texel(f, p, reprojt::v4(c.x, c.y, c.z, c.w), rg, rl);
    out[i] = make_float4(o.x, o.y, o.z, o.w);
}

// grid ceil(N / 256), 256 threads
__global__ __launch_bounds__(256) void k_temporal_to_denoised(const float4* __restrict__ temporal, uint32_t N, float4* __restrict__ out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float4 t = temporal[i];
    out[i] = make_float4(t.x, t.y, t.z, 1.0f);
}
