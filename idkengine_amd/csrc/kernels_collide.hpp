// kernels_collide.hpp — sphere collision queries (idkptCollideSpheres): Intersections.SceneVsMovingSphereCollisionRoutine (Source/Shapes/Intersections.cs:491-593) on the
// resident BVH.  Part of the single translation unit idkpt.hip (included there, in this order); see DESIGN.md §4 for the kernel table.
#pragma once
#include "collide_sphere.hpp"

// k_collide_spheres: one lane per sphere, one wave per workgroup.  The whole routine runs inside the launch — the RecursiveSteps x TestSteps box walks of one sphere depend
// on each other (every walk starts where the previous one pushed the sphere).  The per-sphere arithmetic is collide_sphere.hpp, the text the host build compiles; the walk's
// stack is the lane's LDS column stack[depth][lane] of the traversal kernels (f.stackCap rows for a BLAS, f.tlasCap rows behind them for the TLAS walk), so nothing of it
// lives in scratch.  No atomics: lane i reads sphere i and writes result i.
__global__ __launch_bounds__(WAVE) void k_collide_spheres(DScene s, Frame f, idkpt_collide_settings set, const idkpt_moving_sphere* spheres, idkpt_sphere_collision* out, uint32_t N)
{
    extern __shared__ uint32_t lds[];
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= N) return;
    collide::SceneView v;
    v.nodes = (const collide::F4*)s.nodes; v.triVerts = (const collide::F4*)s.triVerts; v.descs = s.descs; v.instances = s.instances; v.instanceCount = s.instanceCount;
    v.tlas = (const collide::F4*)s.tlas; v.tlasCount = s.tlasCount; v.xforms = (const collide::F4*)s.xforms; v.overflow = s.overflow;
    collide::Stack stack; stack.p = lds + threadIdx.x; stack.stride = WAVE; stack.blasCap = f.stackCap; stack.tlasCap = f.tlasCap;
    const float4* in = (const float4*)(spheres + i);
    const float4 a = in[0], b = in[1], c = in[2];
    idkpt_moving_sphere sp;
    sp.PrevPosition[0] = a.x; sp.PrevPosition[1] = a.y; sp.PrevPosition[2] = a.z; sp.Radius = a.w;
    sp.Position[0] = b.x; sp.Position[1] = b.y; sp.Position[2] = b.z; sp._pad0 = 0u;
    sp.Velocity[0] = c.x; sp.Velocity[1] = c.y; sp.Velocity[2] = c.z; sp._pad1 = 0u;
    const idkpt_sphere_collision r = collide::collide_sphere(v, stack, set, sp);
    float4* o = (float4*)(out + i);
    o[0] = make_float4(r.Position[0], r.Position[1], r.Position[2], __uint_as_float(r.HitCount));
    o[1] = make_float4(r.Velocity[0], r.Velocity[1], r.Velocity[2], __uint_as_float(r.TriangleId));
    o[2] = make_float4(r.Center[0], r.Center[1], r.Center[2], __uint_as_float(r.BlasInstanceId));
    o[3] = make_float4(r.SlidingNormal[0], r.SlidingNormal[1], r.SlidingNormal[2], r.PenetrationDepth);
    o[4] = make_float4(r.TriNormal[0], r.TriNormal[1], r.TriNormal[2], r.Distance);
    o[5] = make_float4(r.TriCollidingPoint[0], r.TriCollidingPoint[1], r.TriCollidingPoint[2], 0.0f);
}
