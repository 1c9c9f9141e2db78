// denoise_variance_host.cpp — the per-pixel functions of idkengine_amd/csrc/denoise_variance_texel.hpp (what the device kernels of kernels_denoise_variance.hpp call)
// compiled for the HOST and run over a whole frame the way host_denoise_variance.hpp runs the launches: tests/test_denoise_variance_ref.py builds this with
// g++ -ffp-contract=off -fsanitize=address,undefined and compares the image with tests/denoise_variance_ref.py's binary32 restatement bit for bit.
//   denoise_variance_host IN OUT
// IN:  int32 W, H, Iterations, DemodulateAlbedo, N; float LumaSigma, VarianceEpsilon, AlbedoSigma, NormalSigma; then Result, Albedo, Normal, Moments: W * H * 4 floats each.
// OUT: W * H * 4 floats (rgb, 1.0).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/denoise_variance_texel.hpp"

using namespace denoisevt;

struct HostFetch {                       // as kernels_denoise_variance.hpp MemFetch: the state image holds (c.rgb, v)
    const float* c; const float* a; const float* n; int W;
    void operator()(int x, int y, State* os, V3* oa, V3* on) const
    {
        const size_t i = ((size_t)y * (size_t)W + (size_t)x) * 4;
        os->c = v3(c[i], c[i + 1], c[i + 2]); os->v = c[i + 3];
        *oa = v3(a[i], a[i + 1], a[i + 2]); *on = v3(n[i], n[i + 1], n[i + 2]);
    }
    float variance(int x, int y) const { return c[((size_t)y * (size_t)W + (size_t)x) * 4 + 3]; }
};

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: denoise_variance_host IN OUT\n"); return 1; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    int32_t hdr[5]; float sig[4];
    if (fread(hdr, 4, 5, in) != 5 || fread(sig, 4, 4, in) != 4) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1], iterations = hdr[2], demod = hdr[3], samples = hdr[4];
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || iterations < 1 || iterations > denoiset::MAX_ITERATIONS || (demod != 0 && demod != 1) || samples < 2) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t N = (size_t)W * H * 4;
    std::vector<float> result(N), albedo(N), normal(N), moments(N);
    if (fread(result.data(), 4, N, in) != N || fread(albedo.data(), 4, N, in) != N || fread(normal.data(), 4, N, in) != N || fread(moments.data(), 4, N, in) != N) { fprintf(stderr, "short images\n"); return 1; }
    fclose(in);

    // the staging of the first launch: the state (c0, v0) of every pixel
    std::vector<float> first(N), ping[2] = {std::vector<float>(N), std::vector<float>(N)};
    for (size_t k = 0; k < N; k += 4) {
        const State st = first_state(v3(result[k], result[k + 1], result[k + 2]), moments[k], moments[k + 1], (uint32_t)samples, v3(albedo[k], albedo[k + 1], albedo[k + 2]), demod != 0);
        first[k] = st.c.x; first[k + 1] = st.c.y; first[k + 2] = st.c.z; first[k + 3] = st.v;
    }
    const float ls2 = sig[0] * sig[0], eps = sig[1], invA = denoiset::inv_sigma2(sig[2], 0), invN = denoiset::inv_sigma2(sig[3], 0);
    const float* src = first.data();
    for (int i = 0; i < iterations; i++) {
        std::vector<float>& dst = ping[i & 1];
        const HostFetch f = {src, albedo.data(), normal.data(), W};
        for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
            State r = atrous_variance_texel(f, W, H, x, y, 1 << i, ls2, eps, invA, invN);
            const size_t k = ((size_t)y * W + x) * 4;
            if (i == iterations - 1) {
                if (demod) r.c = denoiset::remodulate(r.c, v3(albedo[k], albedo[k + 1], albedo[k + 2]));
                r.v = 1.0f;
            }
            dst[k] = r.c.x; dst[k + 1] = r.c.y; dst[k + 2] = r.c.z; dst[k + 3] = r.v;
        }
        src = dst.data();
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    fwrite(src, 4, N, o);
    if (fclose(o) != 0) { perror("close"); return 1; }
    return 0;
}
