// kernels_sky.hpp — the sky's resident faces (DScene::sky: 6 x S x S float4, +X -X +Y -Y +Z -Z) produced on the device: idkptComputeSky / idkptUpdateSky (host side: host_scene.hpp).
// Part of the single translation unit idkpt.hip.
//
// k_sky_atmosphere restates Shaders/AtmosphericScattering/compute.glsl (the engine's default sky, AtmosphericScatterer.Compute: a 128 x 128 RGBA32F cube map) operation
// for operation in binary32, as pt_kernels.hpp restates the shading: same constants, same association of every product and sum, same loop order, same early outs.
// Numerics:
//  * idkpt.hip is compiled with -ffp-contract=off (idkengine_amd/build.py HIPCC_FLAGS): no product and sum below is fused into an fma; every operation rounds once, as written.
//    (The shader's may not be assumed to fuse either; a GL compiler is free to, which is one reason two correct executions differ — see below.)
//  * expf / powf / sqrtf / sinf / cosf and IEEE division only, no fast-math intrinsic.  normalize(v) = v * (1 / sqrt(dot(v, v))) and length(v) = sqrt(dot(v, v)) with
//    dot summed left to right, as everywhere in this library (pt_device.hpp).
//  * The arithmetic subtracts the planet's radius (6 371 000) from lengths near it: one binary32 ulp there is 0.5 m against a 1 200 m Mie scale height, so two correct binary32
//    executions (another exp, another rounding of a dot product) differ far above 1 ulp in the result.  The bound the tests hold this kernel to is therefore measured against
//    the binary64 value of the same formula (tests/test_sky_ref.py, profiles/sky_atmosphere.md), not chosen.
//  * The sun direction, gg and the constant factors of both phase functions do not depend on the texel; every thread computes them from the same inputs with the same
//    operations, so they are the same binary32 values in every thread.
// One thread per texel over 6 S^2 (S need not be a multiple of anything: the last workgroup is cut by the bounds test); ISteps x JSteps inner steps per thread.
#pragma once

namespace skyk {

struct AtmoParams { int ISteps, JSteps; float LightIntensity, Azimuth, Elevation; };   // AtmosphericScatterer.GpuSettings (SettingsUBO of the shader), LightIntensity already max(., 0)

DEV float length3(f3 v) { return sqrtf(dot(v, v)); }
DEV f3 normalize3(f3 v) { const float inv = 1.0f / sqrtf(dot(v, v)); return v * inv; }

// include/Math.glsl:17-39
DEV f3 GetWorldSpaceDirection(float x, float y, int face)
{
    switch (face) {
        case 0: return normalize3(mk3(1.0f, -y, -x));
        case 1: return normalize3(mk3(-1.0f, -y, x));
        case 2: return normalize3(mk3(x, 1.0f, y));
        case 3: return normalize3(mk3(x, -1.0f, -y));
        case 4: return normalize3(mk3(x, -y, 1.0f));
        default: return normalize3(mk3(-x, -y, -1.0f));
    }
}
// include/Math.glsl:139-153 (len = 1.0)
DEV f3 PolarToCartesian(float azimuth, float elevation)
{
    const float sinTheta = sinf(elevation);
    return mk3(sinTheta * cosf(azimuth), cosf(elevation), sinTheta * sinf(azimuth)) * 1.0f;
}
// compute.glsl:51-63: ray-sphere intersection, sphere at the origin; no intersection when x > y
DEV void Rsi(f3 r0, f3 rd, float sr, float* outX, float* outY)
{
    const float a = dot(rd, rd);
    const float b = 2.0f * dot(rd, r0);
    const float c = dot(r0, r0) - sr * sr;
    const float d = b * b - 4.0f * a * c;
    if (d < 0.0f) { *outX = 1e5f; *outY = -1e5f; return; }
    *outX = (-b - sqrtf(d)) / (2.0f * a);
    *outY = (-b + sqrtf(d)) / (2.0f * a);
}
// compute.glsl:65-152
DEV f3 Atmosphere(f3 r, f3 r0, f3 pSun, float iSun, float rPlanet, float rAtmos, f3 kRlh, float kMie, float shRlh, float shMie, float g, int ISteps, int JSteps)
{
    pSun = normalize3(pSun);
    r = normalize3(r);

    float px, py, qx, qy;
    Rsi(r0, r, rAtmos, &px, &py);
    if (px > py) return splat3(0.0f);
    Rsi(r0, r, rPlanet, &qx, &qy);
    py = gmin(py, qx);
    const float IStepsize = (py - px) / (float)ISteps;

    float iTime = 0.0f;
    f3 totalRlh = splat3(0.0f), totalMie = splat3(0.0f);
    float iOdRlh = 0.0f, iOdMie = 0.0f;

    const float mu = dot(r, pSun);
    const float mumu = mu * mu;
    const float gg = g * g;
    const float pRlh = 3.0f / (16.0f * PT_PI) * (1.0f + mumu);
    const float pMie = 3.0f / (8.0f * PT_PI) * ((1.0f - gg) * (mumu + 1.0f)) / (powf(1.0f + gg - 2.0f * mu * g, 1.5f) * (2.0f + gg));

    for (int i = 0; i < ISteps; i++) {
        const f3 iPos = r0 + r * (iTime + IStepsize * 0.5f);
        const float iHeight = length3(iPos) - rPlanet;
        const float odStepRlh = expf(-iHeight / shRlh) * IStepsize;
        const float odStepMie = expf(-iHeight / shMie) * IStepsize;
        iOdRlh += odStepRlh;
        iOdMie += odStepMie;

        float sx, sy;
        Rsi(iPos, pSun, rAtmos, &sx, &sy);
        const float JStepsize = sy / (float)JSteps;
        float jTime = 0.0f, jOdRlh = 0.0f, jOdMie = 0.0f;
        for (int j = 0; j < JSteps; j++) {
            const f3 jPos = iPos + pSun * (jTime + JStepsize * 0.5f);
            const float jHeight = length3(jPos) - rPlanet;
            jOdRlh += expf(-jHeight / shRlh) * JStepsize;
            jOdMie += expf(-jHeight / shMie) * JStepsize;
            jTime += JStepsize;
        }

        const f3 e = -(splat3(kMie * (iOdMie + jOdMie)) + kRlh * (iOdRlh + jOdRlh));
        const f3 attn = mk3(expf(e.x), expf(e.y), expf(e.z));
        totalRlh = totalRlh + odStepRlh * attn;
        totalMie = totalMie + odStepMie * attn;
        iTime += IStepsize;
    }
    return iSun * (pRlh * kRlh * totalRlh + (pMie * kMie) * totalMie);
}

}  // namespace skyk

// compute.glsl:25-49 for texel i of 6 S^2 (face-major, then row, then column: the resident order of DScene::sky)
__global__ __launch_bounds__(256) void k_sky_atmosphere(float4* sky, int S, skyk::AtmoParams p)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t perFace = (uint32_t)S * (uint32_t)S;
    if (i >= 6u * perFace) return;
    const int face = (int)(i / perFace);
    const uint32_t t = i - (uint32_t)face * perFace;
    const int y = (int)(t / (uint32_t)S), x = (int)(t - (uint32_t)y * (uint32_t)S);
    const float u = ((float)x + 0.5f) / (float)S, v = ((float)y + 0.5f) / (float)S;
    const float nx = u * 2.0f - 1.0f, ny = v * 2.0f - 1.0f;
    const f3 toCubemap = skyk::GetWorldSpaceDirection(nx, ny, face);
    const f3 lightPos = skyk::PolarToCartesian(p.Azimuth, p.Elevation);
    const f3 c = skyk::Atmosphere(toCubemap, mk3(0.0f, 6376e3f, 0.0f), lightPos, p.LightIntensity, 6371e3f, 6471e3f, mk3(5.5e-6f, 13.0e-6f, 22.4e-6f), 21e-6f, 8e3f, 1.2e3f, 0.758f, p.ISteps, p.JSteps);
    sky[i] = make_float4(c.x, c.y, c.z, 1.0f);
}

// 8-bit faces (IDKPT_TEXFMT_RGBA8 / SRGB8_A8: what LoadSkyBoxImages holds) -> resident floats, through the texture path's own texel fetch (tex_fetch, pt_kernels.hpp:
// UNORM c / 255; sRGB the 256-entry table on R, G, B, alpha linear): the result is what sampling such a texture with NEAREST returns, bit for bit.
__global__ __launch_bounds__(256) void k_sky_expand(const uint32_t* staged, float4* sky, uint32_t texels, int format, const float* srgbLut)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= texels) return;
    DScene s; s.srgbLut = srgbLut;                                      // (tex_fetch reads nothing else of the scene)
    TexDesc t; t.data = staged; t.w = (int)texels; t.h = 1; t.state = (uint32_t)format << 5; t.pad = 0u;
    sky[i] = tex_fetch(s, t, (int)i, 0);
}
