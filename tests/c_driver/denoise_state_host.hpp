// denoise_state_host.hpp — what denoise_variance_host.cpp and denoise_temporal_host.cpp share: the fetch of a state image and the iterations of
// idkengine_amd/csrc/denoise_variance_texel.hpp over a whole frame, the way host_denoise.hpp's denoise_iterate runs the launches.  Each program makes its own first state.
#pragma once
#include <vector>
#include "../../idkengine_amd/csrc/denoise_variance_texel.hpp"

struct StateFetch {                      // as kernels_denoise_variance.hpp MemFetch: the state image holds (c.rgb, v)
    const float* c; const float* a; const float* n; int W;
    void operator()(int x, int y, denoisevt::State* os, denoiset::V3* oa, denoiset::V3* on) const
    {
        using denoiset::v3;
        const size_t i = ((size_t)y * (size_t)W + (size_t)x) * 4;
        os->c = v3(c[i], c[i + 1], c[i + 2]); os->v = c[i + 3];
        *oa = v3(a[i], a[i + 1], a[i + 2]); *on = v3(n[i], n[i + 1], n[i + 2]);
    }
    float variance(int x, int y) const { return c[((size_t)y * (size_t)W + (size_t)x) * 4 + 3]; }
};

// `iterations` iterations over the W x H frame whose first state is `src` (which may be ping[1]): iteration i writes ping[i & 1], the last one remodulates when `demod`
// and stores alpha 1.  Returns the image the last one wrote.
inline const float* variance_iterations(const float* src, std::vector<float> ping[2], const float* albedo, const float* normal, int W, int H, int iterations, int demod, float ls2, float eps, float invA, float invN)
{
    for (int i = 0; i < iterations; i++) {
        std::vector<float>& dst = ping[i & 1];
        const StateFetch f = {src, albedo, normal, W};
        for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
            denoisevt::State r = denoisevt::atrous_variance_texel(f, W, H, x, y, 1 << i, ls2, eps, invA, invN);
            const size_t k = ((size_t)y * W + x) * 4;
            if (i == iterations - 1) {
                if (demod) r.c = denoiset::remodulate(r.c, denoiset::v3(albedo[k], albedo[k + 1], albedo[k + 2]));
                r.v = 1.0f;
            }
            dst[k] = r.c.x; dst[k + 1] = r.c.y; dst[k + 2] = r.c.z; dst[k + 3] = r.v;
        }
        src = dst.data();
    }
    return src;
}
