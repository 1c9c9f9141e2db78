// collide_sphere.hpp — Intersections.SceneVsMovingSphereCollisionRoutine (Source/Shapes/Intersections.cs:491-593) for ONE sphere, with everything it calls, written once for
// the device (kernels_collide.hpp) and for a host compiler (tests/c_driver/collide_host.cpp builds this file with g++ under ASan/UBSan; tools/collide_bench.py's CPU
// baseline is the same build without the sanitizers).  Depends on <stddef.h>, <stdint.h>, <math.h> and include/idkpt.h only.
//
// Every operation is binary32 in the reference's written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` and sqrtf are the IEEE operations):
//  * Vector3.Dot / Vector3.Distance: x + y + z, left to right; Distance = sqrt of that sum of squares;
//  * (Vector4(p, 1) * Matrix4).Xyz: the order the project fixed for OpenTK in oracle/ref_cpu_baseline.cpp:90-93 (XformRow): (x*m0 + y*m1) + z*m2 + w*m3, left to right,
//    on the GpuMeshTransform rows (row r = column r of the OpenTK matrix);
//  * Vector3.Normalize: scale = 1.0f / sqrtf(dot), then a multiply (oracle/ref_cpu_baseline.cpp:117); Vector3 / float: a division per component;
//  * Vector128.MinNative / MaxNative (Box.GrowToFit): MINPS / MAXPS, `a < b ? a : b` / `a > b ? a : b` — the SECOND operand comes back when either is a NaN.
// The C# half restated here is unpinned (no .NET run stands behind it, like the builder's): these OpenTK orderings are the first place to look if one ever disagrees.
//
// Sphere values never feed an address.  Non-finite centres and radii follow the arithmetic: a NaN centre gives a NaN box, every comparison of BoxVsBox is false and it
// overlaps nothing; a +Inf radius gives the corners +-Inf, which overlap every WORLD-space box (the TLAS nodes), but Box.Transformed multiplies them with the zeros of a
// transform (Inf * 0 = NaN), so the box that enters a BLAS is a NaN box too and the sphere collides with nothing.  A finite radius that covers the scene visits every leaf.
//
// The walk's stack is the caller's: stk[depth * stride] (the device passes its LDS column, stride 64; a host passes an array, stride 1), `blasCap` rows for the walk of
// one BLAS and `tlasCap` rows behind them for the TLAS walk.  BLAS.Intersect(in Box) pushes at most one entry per level — the right child, when both children are inner
// nodes — so it needs max(need(left) + 1, need(right)) <= max(need(left), need(right)) + 1 = BLAS.ComputeRequiredStackSize (Bvh/BLAS.cs:672-702) rows.  A push that finds
// the stack full sets *overflow and the walk of that BLAS / of the TLAS ends at the matching pop (pt_kernels.hpp IntersectBlasAny does the same); it is never dropped silently.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/idkpt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COLLIDE_HD __host__ __device__ inline
#else
#define COLLIDE_HD inline
#endif

namespace collide {

struct alignas(16) F4 { float x, y, z, w; };
struct V3 { float x, y, z; };
struct Box { V3 mn, mx; };

// what the walk reads of the scene: the device's layouts (pt_kernels.hpp DScene), which a host fills from the same arrays
struct SceneView {
    const F4* nodes;            // 2 per GpuBlasNode: {Min.xyz, TriStartOrChild}, {Max.xyz, TriCount}
    const F4* triVerts;         // 3 per BLAS triangle (leaf order): VertexPositions[X], [Y], [Z] of its GpuBlasTriangle (w unused)
    const GpuBlasDesc* descs;
    const GpuBlasInstance* instances; int instanceCount;
    const F4* tlas; int tlasCount;   // 2 per GpuTlasNode: {Min.xyz, IsLeaf:1 | ChildOrInstanceId:31}, {Max.xyz, pad}
    const F4* xforms;           // 9 per GpuMeshTransform: Model rows 0-2, InvModel rows 3-5, PrevModel rows 6-8
    uint32_t* overflow;
};
struct Stack { uint32_t* p; int stride, blasCap, tlasCap; };

COLLIDE_HD V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
COLLIDE_HD V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
COLLIDE_HD V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
COLLIDE_HD V3 mul(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
COLLIDE_HD V3 divs(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
COLLIDE_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
COLLIDE_HD V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
COLLIDE_HD float distance(V3 a, V3 b) { const V3 d = sub(b, a); return sqrtf(d.x * d.x + d.y * d.y + d.z * d.z); }
COLLIDE_HD V3 normalize(V3 v) { const float scale = 1.0f / sqrtf(dot(v, v)); return mul(v, scale); }
COLLIDE_HD float min_native(float a, float b) { return a < b ? a : b; }
COLLIDE_HD float max_native(float a, float b) { return a > b ? a : b; }
COLLIDE_HD uint32_t f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
COLLIDE_HD V3 xyz(const F4& a) { return v3(a.x, a.y, a.z); }

// (Vector4(p, w) * Matrix4).Xyz on three rows of a GpuMeshTransform
COLLIDE_HD V3 xform_rows(const F4* r, V3 p, float w)
{
    return v3((p.x * r[0].x) + (p.y * r[0].y) + (p.z * r[0].z) + (w * r[0].w),
              (p.x * r[1].x) + (p.y * r[1].y) + (p.z * r[1].z) + (w * r[1].w),
              (p.x * r[2].x) + (p.y * r[2].y) + (p.z * r[2].z) + (w * r[2].w));
}

// Intersections.BoxVsBox (Intersections.cs:150-153): a.Min <= b.Max && a.Max >= b.Min on x, y, z
COLLIDE_HD bool box_vs_box(const Box& a, V3 bMin, V3 bMax)
{
    return a.mn.x <= bMax.x && a.mn.y <= bMax.y && a.mn.z <= bMax.z && a.mx.x >= bMin.x && a.mx.y >= bMin.y && a.mx.z >= bMin.z;
}

// Box.Transformed (Shapes/Box.cs:166-175): Box.Empty() (:179-185), the eight corners of the indexer (:28-38) through the matrix, GrowToFit (:40-44)
COLLIDE_HD Box box_transformed(const Box& b, const F4* rows)
{
    Box n; n.mn = v3(3.4028235e+38f, 3.4028235e+38f, 3.4028235e+38f); n.mx = v3(-3.4028235e+38f, -3.4028235e+38f, -3.4028235e+38f);
    for (int i = 0; i < 8; i++) {
        const V3 c = v3((i & 1) ? b.mx.x : b.mn.x, (i & 2) ? b.mx.y : b.mn.y, (i & 4) ? b.mx.z : b.mn.z);
        const V3 p = xform_rows(rows, c, 1.0f);
        n.mn = v3(min_native(n.mn.x, p.x), min_native(n.mn.y, p.y), min_native(n.mn.z, p.z));
        n.mx = v3(max_native(n.mx.x, p.x), max_native(n.mx.y, p.y), max_native(n.mx.z, p.z));
    }
    return n;
}

// Intersections.TriangleClosestPoint (Intersections.cs:38-94), every early return
COLLIDE_HD V3 triangle_closest_point(V3 p0, V3 p1, V3 p2, V3 point)
{
    const V3 ab = sub(p1, p0), ac = sub(p2, p0), ap = sub(point, p0);
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) return p0;
    const V3 bp = sub(point, p1);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) return p1;
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { const float v = d1 / (d1 - d3); return add(p0, mul(ab, v)); }
    const V3 cp = sub(point, p2);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) return p2;
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { const float w = d2 / (d2 - d6); return add(p0, mul(ac, w)); }
    const float va = d3 * d6 - d5 * d4;
    if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) { const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); return add(p1, mul(sub(p2, p1), w)); }
    const float denom = 1.0f / (va + vb + vc);
    const float v = vb * denom, w = vc * denom;
    return add(add(p0, mul(ab, v)), mul(ac, w));
}

// Plane.Project / Plane.Reflect (Shapes/Plane.cs:14-24)
COLLIDE_HD V3 plane_project(V3 v, V3 n) { return sub(v, mul(n, dot(n, v))); }
COLLIDE_HD V3 plane_reflect(V3 v, V3 n) { return sub(v, mul(n, 2.0f * dot(n, v))); }

// the locals the lambda of SceneVsMovingSphere captures (Intersections.cs:532-538), plus the ids of the triangle that holds the best distance
struct StepState {
    V3 center; float radius;
    float bestTriDistance, bestPenetrationDepth; bool triCollisionDetected;
    V3 slidingNormal, triNormal, triCollidingPoint; uint32_t triangleId, blasInstanceId;
};

// the per-triangle callback (Intersections.cs:539-581)
COLLIDE_HD void visit_triangle(const SceneView& s, StepState& st, uint32_t blasInstanceId, uint32_t triangleId)
{
    const GpuBlasInstance inst = s.instances[blasInstanceId];
    const F4* tv = s.triVerts + 3 * (size_t)triangleId;
    const F4 a = tv[0], b = tv[1], c = tv[2];
    const F4* model = s.xforms + 9 * (size_t)inst.MeshTransformId;            // Triangle.Transformed (Triangle.cs:40-45): ModelMatrix, not the inverse
    const V3 p0 = xform_rows(model, xyz(a), 1.0f), p1 = xform_rows(model, xyz(b), 1.0f), p2 = xform_rows(model, xyz(c), 1.0f);
    const V3 closest = triangle_closest_point(p0, p1, p2, st.center);          // SphereVsTriangle (:134-141)
    const float dist = distance(closest, st.center);
    const float penetrationDepth = st.radius - dist;
    const bool intersects = penetrationDepth > 0.0f;
    if (!intersects || dist >= st.bestTriDistance) return;                     // (the first triangle visited keeps a tie)
    if (dist == 0.0f) return;
    st.triCollisionDetected = true;
    V3 triFaceNormal = normalize(cross(sub(p1, p0), sub(p2, p0)));             // Triangle.Normal (Triangle.cs:12)
    const V3 hitPointToSphereDir = divs(sub(st.center, closest), dist);
    const float cosTheta = dot(triFaceNormal, hitPointToSphereDir);
    if (cosTheta < 0.0f) triFaceNormal = mul(triFaceNormal, -1.0f);
    st.slidingNormal = hitPointToSphereDir; st.triNormal = triFaceNormal; st.triCollidingPoint = closest;
    st.bestTriDistance = dist; st.bestPenetrationDepth = penetrationDepth;
    st.triangleId = triangleId; st.blasInstanceId = blasInstanceId;
}

// BLAS.Intersect(blas, geometry, Box, func) (Bvh/BLAS.cs:388-439) for BLAS instance `blasInstanceId`, the box already in its local space
COLLIDE_HD void blas_box_walk(const SceneView& s, const Stack& stack, StepState& st, const Box& box, uint32_t blasInstanceId)
{
    const GpuBlasDesc& d = s.descs[s.instances[blasInstanceId].BlasId];
    const uint32_t triangleOffset = (uint32_t)d.TriangleOffset;
    const F4* nodes = s.nodes + 2 * (size_t)d.NodeOffset;
    { const F4 rmin = nodes[2], rmax = nodes[3]; if (!box_vs_box(box, xyz(rmin), xyz(rmax))) return; }
    int sp = 0;
    uint32_t top = 2u;
    while (true) {
        const F4* p = nodes + 2 * (size_t)top;
        const F4 lmin = p[0], lmax = p[1], rmin = p[2], rmax = p[3];
        const uint32_t lStart = f32_bits(lmin.w), lCount = f32_bits(lmax.w), rStart = f32_bits(rmin.w), rCount = f32_bits(rmax.w);
        const bool hitLeft = box_vs_box(box, xyz(lmin), xyz(lmax)), hitRight = box_vs_box(box, xyz(rmin), xyz(rmax));
        const bool intersectLeft = hitLeft && lCount > 0u, intersectRight = hitRight && rCount > 0u;
        if (intersectLeft || intersectRight) {
            const uint32_t first = intersectLeft ? lStart : rStart;
            const uint32_t end = !intersectRight ? (first + lCount) : (rStart + rCount);
            for (uint32_t i = first; i < end; i++) visit_triangle(s, st, blasInstanceId, triangleOffset + i);
        }
        const bool traverseLeft = hitLeft && lCount == 0u, traverseRight = hitRight && rCount == 0u;
        if (traverseLeft || traverseRight) {
            top = traverseLeft ? lStart : rStart;
            if (traverseLeft && traverseRight) { if (sp < stack.blasCap) stack.p[(size_t)sp * stack.stride] = rStart; else *s.overflow = 1u; sp++; }
        } else {
            if (sp == 0) break;
            sp--;
            if (sp >= stack.blasCap) break;                                    // the matching push was flagged: stop instead of following a garbage index
            top = stack.p[(size_t)sp * stack.stride];
        }
    }
}

// BVH.Intersect(in Box, func) (Bvh/BVH.cs:196-223): the instance loop (:204-221), or TLAS.Intersect (Bvh/TLAS.cs:209-264) when asked for
COLLIDE_HD void scene_box_walk(const SceneView& s, const Stack& stack, StepState& st, const Box& box, bool useTlas)
{
    if (!useTlas) {
        for (int i = 0; i < s.instanceCount; i++) {
            const Box local = box_transformed(box, s.xforms + 9 * (size_t)s.instances[i].MeshTransformId + 3);
            blas_box_walk(s, stack, st, local, (uint32_t)i);
        }
        return;
    }
    if (s.tlasCount == 0) return;
    uint32_t* tstk = stack.p + (size_t)stack.blasCap * stack.stride;           // the TLAS rows follow the BLAS rows
    int sp = 0;
    uint32_t top = 0u;
    while (true) {
        const uint32_t packed = f32_bits(s.tlas[2 * (size_t)top].w), id = packed & 0x7fffffffu;
        if ((packed >> 31) == 1u) {
            const Box local = box_transformed(box, s.xforms + 9 * (size_t)s.instances[id].MeshTransformId + 3);
            blas_box_walk(s, stack, st, local, id);
            if (sp == 0) break;
            sp--;
            if (sp >= stack.tlasCap) break;
            top = tstk[(size_t)sp * stack.stride];
            continue;
        }
        const uint32_t l = id, r = id + 1u;
        const F4 lmin = s.tlas[2 * (size_t)l], lmax = s.tlas[2 * (size_t)l + 1], rmin = s.tlas[2 * (size_t)r], rmax = s.tlas[2 * (size_t)r + 1];
        Box nl, nr; nl.mn = xyz(lmin); nl.mx = xyz(lmax); nr.mn = xyz(rmin); nr.mx = xyz(rmax);
        const bool traverseLeft = box_vs_box(nl, box.mn, box.mx), traverseRight = box_vs_box(nr, box.mn, box.mx);   // (:247-248: the node is the first operand)
        if (traverseLeft || traverseRight) {
            top = traverseLeft ? l : r;
            if (traverseLeft && traverseRight) { if (sp < stack.tlasCap) tstk[(size_t)sp * stack.stride] = r; else *s.overflow = 1u; sp++; }
        } else {
            if (sp == 0) break;
            sp--;
            if (sp >= stack.tlasCap) break;
            top = tstk[(size_t)sp * stack.stride];
        }
    }
}

// SceneVsMovingSphere (Intersections.cs:521-593): true when a step collided; `center` is the ref parameter movingSphere.Center
COLLIDE_HD bool scene_vs_moving_sphere(const SceneView& s, const Stack& stack, bool useTlas, int testSteps, V3 destination, V3& center, float radius, StepState& hit)
{
    const V3 stepSize = divs(sub(destination, center), (float)testSteps);
    for (int i = 0; i < testSteps; i++) {
        center = add(center, stepSize);
        Box hitBox; hitBox.mn = sub(center, v3(radius, radius, radius)); hitBox.mx = add(center, v3(radius, radius, radius));
        StepState st;
        st.center = center; st.radius = radius; st.bestTriDistance = 3.4028235e+38f; st.bestPenetrationDepth = 0.0f; st.triCollisionDetected = false;
        st.slidingNormal = st.triNormal = st.triCollidingPoint = v3(0.0f, 0.0f, 0.0f); st.triangleId = st.blasInstanceId = 0xFFFFFFFFu;
        scene_box_walk(s, stack, st, hitBox, useTlas);
        if (st.triCollisionDetected) {
            center = add(center, mul(st.slidingNormal, st.bestPenetrationDepth));
            hit = st;
            return true;
        }
    }
    return false;
}

// SceneVsMovingSphereCollisionRoutine (Intersections.cs:492-507) with the caller's callback inside: Response 0 none, 1 Camera.CollisionDetection's slide
// (Camera.cs:158-167, Plane.Project), 2 LightManager.CollisionDetection's bounce (Render/LightManager.cs:247-256, Plane.Reflect) — the three assignments of either
COLLIDE_HD idkpt_sphere_collision collide_sphere(const SceneView& s, const Stack& stack, const idkpt_collide_settings& set, const idkpt_moving_sphere& in)
{
    V3 center = v3(in.PrevPosition[0], in.PrevPosition[1], in.PrevPosition[2]), position = v3(in.Position[0], in.Position[1], in.Position[2]);
    V3 velocity = v3(in.Velocity[0], in.Velocity[1], in.Velocity[2]), prevSpherePos = center;
    StepState last;
    last.slidingNormal = last.triNormal = last.triCollidingPoint = v3(0.0f, 0.0f, 0.0f); last.bestPenetrationDepth = 0.0f; last.bestTriDistance = 0.0f;
    last.triangleId = last.blasInstanceId = 0xFFFFFFFFu;
    uint32_t hitCount = 0u;
    for (int i = 0; i < set.RecursiveSteps; i++) {
        StepState h;
        if (!scene_vs_moving_sphere(s, stack, set.UseTlas != 0, set.TestSteps, position, center, in.Radius, h)) break;
        center = add(center, mul(h.slidingNormal, set.EpsilonNormalOffset));
        if (set.Response == 1) {
            const V3 deltaStep = sub(position, prevSpherePos);
            position = add(center, plane_project(deltaStep, h.slidingNormal));
            velocity = plane_project(velocity, h.slidingNormal);
            prevSpherePos = center;
        } else if (set.Response == 2) {
            const V3 deltaStep = sub(position, prevSpherePos);
            position = add(center, plane_reflect(deltaStep, h.slidingNormal));
            velocity = plane_reflect(velocity, h.slidingNormal);
            prevSpherePos = center;
        }
        last = h; hitCount++;
    }
    idkpt_sphere_collision o;
    o.Position[0] = position.x; o.Position[1] = position.y; o.Position[2] = position.z; o.HitCount = hitCount;
    o.Velocity[0] = velocity.x; o.Velocity[1] = velocity.y; o.Velocity[2] = velocity.z; o.TriangleId = last.triangleId;
    o.Center[0] = center.x; o.Center[1] = center.y; o.Center[2] = center.z; o.BlasInstanceId = last.blasInstanceId;
    o.SlidingNormal[0] = last.slidingNormal.x; o.SlidingNormal[1] = last.slidingNormal.y; o.SlidingNormal[2] = last.slidingNormal.z; o.PenetrationDepth = last.bestPenetrationDepth;
    o.TriNormal[0] = last.triNormal.x; o.TriNormal[1] = last.triNormal.y; o.TriNormal[2] = last.triNormal.z; o.Distance = last.bestTriDistance;
    o.TriCollidingPoint[0] = last.triCollidingPoint.x; o.TriCollidingPoint[1] = last.triCollidingPoint.y; o.TriCollidingPoint[2] = last.triCollidingPoint.z; o._pad = 0u;
    return o;
}

} // namespace collide
