// reproject_texel.hpp — the per-pixel arithmetic of idkptCaptureGeometry's record and of idkptReproject (the contract of include/idkpt.h, "temporal reprojection"): the
// geometry record of a centre ray and its hit, and the blend of one pixel of the current frame with the history frame's temporal image found through the history frame's
// camera.  Written once for the device (kernels_reproject.hpp) and for a host compiler (tests/c_driver/reproject_host.cpp builds this file with g++ under ASan/UBSan).
// Depends on <math.h>, <stdint.h> and <string.h> only.  No counterpart in the reference.
//
// Every operation is a binary32 + - * / or floorf in the written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` is the IEEE division), so
// tests/reproject_ref.py restates the same text in numpy and is compared bit for bit.  The only values that feed an address are x0, y0 = floorf(u), floorf(v), taken after
// `u > -1 && u < W && v > -1 && v < H` held (false for NaN), and every tap is tested against the image before it is fetched.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REPROJECT_HD __host__ __device__ inline
#else
#define REPROJECT_HD inline
#endif

namespace reprojt {

struct V4 { float x, y, z, w; };
REPROJECT_HD V4 v4(float x, float y, float z, float w) { V4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

constexpr uint32_t MISS_ID = 0xFFFFFFFFu;          // the id bits of a pixel whose centre ray left the scene
constexpr float FLOAT_MAX = 3.402823466e+38f;
constexpr float MIN_WEIGHT = 0.01f;                // the valid taps must carry at least this much of the bilinear footprint

REPROJECT_HD uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
REPROJECT_HD float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
REPROJECT_HD bool finite(float c) { return fabsf(c) <= FLOAT_MAX; }           // false for NaN and for either infinity

// the geometry record of a pixel: the world position of the centre ray's closest hit and the instance it belongs to, or the ray's direction and MISS_ID
REPROJECT_HD V4 pack_record(const float* o, const float* d, float T, uint32_t meshTransformId, bool hit)
{
    if (!hit) return v4(d[0], d[1], d[2], float_of(MISS_ID));
    return v4(o[0] + d[0] * T, o[1] + d[1] * T, o[2] + d[2] * T, float_of(meshTransformId));
}

struct Params {
    int W, H;
    float M[16];               // PrevProjView of the history frame, OpenTK memory order: clip_j = p . column j
    float prevPos[3];          // PrevViewPos
    float tol2;                // PositionTolerance * PositionTolerance, computed once per call on the host in binary32
    float maxHistory;
    float n;                   // (float) of the slot's accumulated sample count, >= 1
};

REPROJECT_HD float dist2(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// One pixel.  cur = Result of the slot, g = its geometry record, l = its LOOKUP record: the point that is looked up in the history frame — g itself, or the slot's motion
// record (motion_texel.hpp: where the surface stood when the history was captured; idkptCaptureMotion).  g supplies the id, l the position in the clip coordinates, in
// the limit and in the tap test.  fetch(qx, qy, &hg, &hc) returns the history slot's geometry record and temporal texel of an IN-IMAGE position and is never called for
// one outside.  Returns (rgb, effective sample count).
template <class Fetch>
REPROJECT_HD V4 reproject_texel(const Fetch& fetch, const Params& P, V4 cur, V4 g, V4 l)
{
    const V4 none = v4(cur.x, cur.y, cur.z, P.n);
    const uint32_t id = bits_of(g.w);
    const bool miss = id == MISS_ID;
    const float* M = P.M;
    float cx = (l.x * M[0] + l.y * M[4]) + l.z * M[8];
    float cy = (l.x * M[1] + l.y * M[5]) + l.z * M[9];
    float cw = (l.x * M[3] + l.y * M[7]) + l.z * M[11];
    if (!miss) { cx = cx + M[12]; cy = cy + M[13]; cw = cw + M[15]; }          // a miss is a direction: w = 0
    if (!(cw > 0.0f)) return none;
    const float u = (cx / cw * 0.5f + 0.5f) * (float)P.W - 0.5f;
    const float v = (cy / cw * 0.5f + 0.5f) * (float)P.H - 0.5f;
    if (!(u > -1.0f && u < (float)P.W && v > -1.0f && v < (float)P.H)) return none;   // (NaN lands here)
    const float x0f = floorf(u), y0f = floorf(v);
    const float fx = u - x0f, fy = v - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;                                     // -1 .. W - 1, -1 .. H - 1
    const float wt[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
    const float limit = miss ? 0.0f : P.tol2 * dist2(l.x, l.y, l.z, P.prevPos[0], P.prevPos[1], P.prevPos[2]);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, sumW = 0.0f;
    for (int k = 0; k < 4; k++) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
        V4 hg, hc;
        fetch(qx, qy, &hg, &hc);
        if (bits_of(hg.w) != id) continue;
        if (!miss && !(dist2(l.x, l.y, l.z, hg.x, hg.y, hg.z) <= limit)) continue;   // (false for a NaN on either side)
        if (!(finite(hc.x) && finite(hc.y) && finite(hc.z) && finite(hc.w))) continue;
        const float w = wt[k];
        sr = sr + hc.x * w; sg = sg + hc.y * w; sb = sb + hc.z * w; sa = sa + hc.w * w;
        sumW = sumW + w;
    }
    if (!(sumW >= MIN_WEIGHT)) return none;
    const float hr = sr / sumW, hgr = sg / sumW, hb = sb / sumW, ha = sa / sumW;
    const float Hc = fminf(ha, P.maxHistory);
    const float den = Hc + P.n;
    return v4((hr * Hc + cur.x * P.n) / den, (hgr * Hc + cur.y * P.n) / den, (hb * Hc + cur.z * P.n) / den, den);
}

// ... without a motion record: the geometry record is looked up
template <class Fetch>
REPROJECT_HD V4 reproject_texel(const Fetch& fetch, const Params& P, V4 cur, V4 g) { return reproject_texel(fetch, P, cur, g, g); }

// One pixel of idkptReprojectMoments: the same clip coordinates, taps, validity rules and blend on the luminance moments.  (m1, m2) of the slot's moments image, g its
// geometry record, l its lookup record; fetch returns the history slot's geometry record and TEMPORAL MOMENTS texel (M1, M2, 0, cnt).  Returns (M1, M2, 0, effective
// sample count): the third channel is stored as 0 whatever the history held there.
template <class Fetch>
REPROJECT_HD V4 reproject_moments_texel(const Fetch& fetch, const Params& P, float m1, float m2, V4 g, V4 l)
{
    V4 o = reproject_texel(fetch, P, v4(m1, m2, 0.0f, 0.0f), g, l);
    o.z = 0.0f;
    return o;
}
template <class Fetch>
REPROJECT_HD V4 reproject_moments_texel(const Fetch& fetch, const Params& P, float m1, float m2, V4 g) { return reproject_moments_texel(fetch, P, m1, m2, g, g); }

}  // namespace reprojt
