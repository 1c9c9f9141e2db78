// noise_host.cpp — the per-texel functions of idkengine_amd/csrc/noise_texel.hpp (what k_final_draw_noise and k_noise_estimate call) compiled for the HOST and run over a
// whole frame the way the kernels run them: tests/test_noise_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares moments, tile map and
// summary with tests/noise_ref.py's binary32 restatement bit for bit.
//   noise_host IN OUT
// IN:  int32 W, H, K, n; uint32 accumulated; float Epsilon, Threshold; the moments image the fold starts from (W * H * 4 floats: m1, m2, 0, 1); then K radiance images
//      (W * H * 4 floats each), folded in order with the weights of accumulated, accumulated + 1, ...
// OUT: the moments image after the fold (W * H * 4 floats); the tile map of an estimate over n samples (tilesX * tilesY * 2 floats); the summary (4 dwords).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/noise_texel.hpp"

using namespace noiset;

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: noise_host IN OUT\n"); return 1; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    int32_t hdr[4]; uint32_t accumulated; float par[2];
    if (fread(hdr, 4, 4, in) != 4 || fread(&accumulated, 4, 1, in) != 1 || fread(par, 4, 2, in) != 2) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1], K = hdr[2], n = hdr[3];
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || K < 0 || K > 256 || n < 2) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t N = (size_t)W * H;
    std::vector<float> mom(N * 4), nr(N * 4);
    if (fread(mom.data(), 4, N * 4, in) != N * 4) { fprintf(stderr, "short moments\n"); return 1; }
    for (int k = 0; k < K; k++) {                         // FinalDraw's loop over the samples of a batch
        if (fread(nr.data(), 4, N * 4, in) != N * 4) { fprintf(stderr, "short sample\n"); return 1; }
        const float w = 1.0f / ((float)(accumulated + (uint32_t)k) + 1.0f);
        for (size_t i = 0; i < N; i++) {
            float m1 = mom[4 * i], m2 = mom[4 * i + 1];
            fold(&m1, &m2, luminance(nr[4 * i], nr[4 * i + 1], nr[4 * i + 2]), w);
            mom[4 * i] = m1; mom[4 * i + 1] = m2; mom[4 * i + 2] = 0.0f; mom[4 * i + 3] = 1.0f;
        }
    }
    fclose(in);

    const int tilesX = (W + TILE - 1) / TILE, tilesY = (H + TILE - 1) / TILE;
    std::vector<float> tiles((size_t)tilesX * tilesY * 2);
    uint32_t summary[4] = {0u, 0u, (uint32_t)(tilesX * tilesY), (uint32_t)n};
    for (int ty = 0; ty < tilesY; ty++) for (int tx = 0; tx < tilesX; tx++) {   // k_noise_estimate: one wave per tile, lane j = (y & 7) * 8 + (x & 7)
        float e[TILE_TEXELS]; uint8_t inside[TILE_TEXELS];
        for (int j = 0; j < TILE_TEXELS; j++) {
            const int x = tx * TILE + (j & 7), y = ty * TILE + (j >> 3);
            inside[j] = x < W && y < H; e[j] = 0.0f;
            if (inside[j]) { const size_t i = (size_t)y * W + x; e[j] = pixel_error(mom[4 * i], mom[4 * i + 1], (uint32_t)n, par[0]); }
        }
        float mean, mx;
        tile_reduce(e, inside, &mean, &mx);
        const size_t t = (size_t)ty * tilesX + tx;
        tiles[2 * t] = mean; tiles[2 * t + 1] = mx;
        if (mean > par[1]) summary[0]++;
        uint32_t b; memcpy(&b, &mean, 4);
        if (b > summary[1]) summary[1] = b;               // the atomic max on the bit pattern of a non-negative float
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    fwrite(mom.data(), 4, N * 4, o); fwrite(tiles.data(), 4, tiles.size(), o); fwrite(summary, 4, 4, o);
    if (fclose(o) != 0) { perror("close"); return 1; }
    return 0;
}
