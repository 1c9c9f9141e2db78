// motion_texel.hpp — the per-pixel arithmetic of idkptCaptureMotion's motion record (the contract of include/idkpt.h, "motion-aware capture"): where the surface point a
// pixel's centre ray hit stood in the PREVIOUS frame — the hit's barycentrics applied to the previous local positions of its triangle's vertices, taken to the world
// through the PrevModel of its instance.  Written once for the device (kernels_reproject.hpp, k_geom_motion_pack) and for a host compiler
// (tests/c_driver/motion_host.cpp builds this file with g++ under ASan/UBSan).  Depends on reproject_texel.hpp only.  The reference's rasterizer derives its motion vectors
// from the same inputs (GBuffer/VertexPath/vertex.glsl: PrevProjView * prevModelMatrix * prevVertexPosition); its path tracer has no counterpart.
//
// Every operation is a binary32 + - * in the written order (the library is compiled with -ffp-contract=off: nothing is fused), so tests/motion_ref.py restates the same
// text in numpy and is compared bit for bit.  Nothing here feeds an address: the caller fetches q0 .. q2 and the three rows after checking the ids against the tables.
#pragma once
#include "reproject_texel.hpp"

namespace motiont {

using reprojt::V4;

// b = (bx, by, (1 - bx) - by) weighs vertex x, y, z of the triangle (ShadeHit's convention); q_k: the previous local position of vertex k; r0 .. r2: the three rows of
// PrevModel (rows 6-8 of the nine float4 of a GpuMeshTransform: world = (row . local) + row.w).  Returns (p'.x, p'.y, p'.z, bits(meshTransformId)).
// A NaN or an infinity in a position or in PrevModel is carried into the record: idkptReproject's existing rules then give the pixel no history.
REPROJECT_HD V4 prev_record(float bx, float by, const float* q0, const float* q1, const float* q2, V4 r0, V4 r1, V4 r2, uint32_t meshTransformId)
{
    const float bz = (1.0f - bx) - by;
    const float lx = (q0[0] * bx + q1[0] * by) + q2[0] * bz;
    const float ly = (q0[1] * bx + q1[1] * by) + q2[1] * bz;
    const float lz = (q0[2] * bx + q1[2] * by) + q2[2] * bz;
    return reprojt::v4(((r0.x * lx + r0.y * ly) + r0.z * lz) + r0.w, ((r1.x * lx + r1.y * ly) + r1.z * lz) + r1.w, ((r2.x * lx + r2.y * ly) + r2.z * lz) + r2.w,
                       reprojt::float_of(meshTransformId));
}

// Can the record of a hit be gathered at all?  The closest-hit core only returns ids of the resident tables; a hit record that does not (device memory a host wrote
// itself) stores the geometry record instead of reading outside.
REPROJECT_HD bool ids_resident(uint32_t tri, uint32_t triCount, uint32_t meshTransformId, uint32_t xformCount) { return tri < triCount && meshTransformId < xformCount; }
REPROJECT_HD bool vertices_resident(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t vertexCount) { return v0 < vertexCount && v1 < vertexCount && v2 < vertexCount; }

}  // namespace motiont
