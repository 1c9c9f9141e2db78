// denoise_variance_host.cpp — the per-pixel functions of idkengine_amd/csrc/denoise_variance_texel.hpp (what the device kernels of kernels_denoise_variance.hpp call)
// compiled for the HOST and run over a whole frame the way host_denoise_variance.hpp runs the launches (the iterations: denoise_state_host.hpp):
// tests/test_denoise_variance_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares the image with tests/denoise_variance_ref.py's binary32 restatement bit for bit.
//   denoise_variance_host IN OUT
// IN:  int32 W, H, Iterations, DemodulateAlbedo, N; float LumaSigma, VarianceEpsilon, AlbedoSigma, NormalSigma; then Result, Albedo, Normal, Moments: W * H * 4 floats each.
// OUT: W * H * 4 floats (rgb, 1.0).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "denoise_state_host.hpp"

using namespace denoisevt;

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
    const float* src = variance_iterations(first.data(), ping, albedo.data(), normal.data(), W, H, iterations, demod, ls2, eps, invA, invN);
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    fwrite(src, 4, N, o);
    if (fclose(o) != 0) { perror("close"); return 1; }
    return 0;
}
