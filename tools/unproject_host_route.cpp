// unproject_host_route.cpp — the route a host had before idkptUnprojectSky: the per-texel functions of idkengine_amd/csrc/unproject_texel.hpp on CPU threads, producing
// the RGBA32F faces idkptUpdateSky takes.  Built by tools/unproject_timing.py (g++ -O2 -ffp-contract=off -fopenmp -shared); a measuring aid, not part of the product.
#include <stdint.h>
#include <vector>
#include "../idkengine_amd/csrc/unproject_texel.hpp"

extern "C" void host_unproject(const float* pixels, int W, int H, int ch, int S, float* faces, int threads)
{
    using namespace unprojt;
    std::vector<uint16_t> pano((size_t)W * H * 4);
#pragma omp parallel for num_threads(threads) schedule(static)
    for (long t = 0; t < (long)W * H; t++) {
        const float* s = pixels + (size_t)t * ch;
        const H4 h = pack_texel(s[0], s[1], s[2], ch == 4 ? s[3] : 1.0f);
        pano[(size_t)t * 4] = h.x; pano[(size_t)t * 4 + 1] = h.y; pano[(size_t)t * 4 + 2] = h.z; pano[(size_t)t * 4 + 3] = h.w;
    }
    const HalfImage src = {pano.data(), W};
#pragma omp parallel for num_threads(threads) schedule(static)
    for (long r = 0; r < 6L * S; r++) {
        const int f = (int)(r / S), y = (int)(r % S);
        for (int x = 0; x < S; x++) {
            const V4 v = expand_half(store_texel(unproject_value(src, W, H, x, y, f, S)));
            float* o = faces + (((size_t)f * S + y) * S + x) * 4;
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        }
    }
}
