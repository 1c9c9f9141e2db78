// bloom_host.cpp — the per-texel functions of idkengine_amd/csrc/bloom_texel.hpp (what the device kernels of kernels_bloom.hpp call) compiled for the HOST and run over
// a whole frame: tests/test_bloom_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares every level and the expanded image with
// tests/bloom_ref.py's binary32 restatement bit for bit.
//   bloom_host IN OUT
// IN:  int32 W, H, MinusLods; float Threshold, MaxColor; then W * H * 4 floats (the RGBA32F image).
// OUT: int32 levels; the down levels 0 .. levels - 1, the up levels 0 .. levels - 2 (w * h * 4 uint16 each, sizes by bloom_levels / level_dim); W * H * 4 floats (expanded).
// Additionally checks f32_to_f16_rtz against a list of values whose halves are known (exit status 2 on a mismatch).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/bloom_texel.hpp"

using namespace bloomt;

static void store(std::vector<uint16_t>& lvl, int w, int x, int y, V3 v)
{
    uint16_t* t = &lvl[((size_t)y * w + x) * 4];
    t[0] = f32_to_f16_rtz(v.x); t[1] = f32_to_f16_rtz(v.y); t[2] = f32_to_f16_rtz(v.z); t[3] = 0x3C00;
}

static int self_check()
{
    struct { float f; uint16_t h; } k[] = {
        {0.0f, 0x0000}, {-0.0f, 0x8000}, {1.0f, 0x3C00}, {1.0009765625f, 0x3C01}, {1.00097644329071044921875f, 0x3C00} /* just below the next half */, {1.0f + 0.9f / 1024.0f, 0x3C00},
        {1.00146484375f, 0x3C01} /* a tie: toward zero */, {-1.00146484375f, 0xBC01}, {65504.0f, 0x7BFF}, {65519.0f, 0x7BFF}, {65520.0f, 0x7BFF}, {65536.0f, 0x7BFF}, {70000.0f, 0x7BFF}, {3.0e38f, 0x7BFF},
        {-70000.0f, 0xFBFF}, {6.103515625e-5f, 0x0400} /* the smallest normal half */, {6.1e-5f, 0x03FF}, {5.9604644775390625e-8f, 0x0001}, {1.1e-7f, 0x0001}, {5.9e-8f, 0x0000}, {1e-30f, 0x0000}, {-1.5e-7f, 0x8002},
    };
    for (auto& c : k) if (f32_to_f16_rtz(c.f) != c.h) { fprintf(stderr, "f32_to_f16_rtz(%a) = %04x, want %04x\n", c.f, f32_to_f16_rtz(c.f), c.h); return 2; }
    for (uint32_t h = 0; h < 0x10000u; h++) {                 // every finite half survives the round trip
        if (((h >> 10) & 31u) == 31u) continue;
        if (f32_to_f16_rtz(f16_to_f32((uint16_t)h)) != h) { fprintf(stderr, "round trip of half %04x\n", h); return 2; }
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (self_check()) return 2;
    if (argc != 3) { fprintf(stderr, "usage: bloom_host IN OUT\n"); return 1; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    int32_t hdr[3]; float set[2];
    if (fread(hdr, 4, 3, in) != 3 || fread(set, 4, 2, in) != 2) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1], minusLods = hdr[2];
    if (W < 2 || H < 2 || W > 4096 || H > 4096 || minusLods < 0) { fprintf(stderr, "bad sizes\n"); return 1; }
    std::vector<float> img((size_t)W * H * 4);
    if (fread(img.data(), 4, img.size(), in) != img.size()) { fprintf(stderr, "short image\n"); return 1; }
    fclose(in);

    int w0 = 0, h0 = 0;
    const int levels = bloom_levels(W, H, minusLods, &w0, &h0);
    std::vector<std::vector<uint16_t>> down(levels), up(levels - 1);
    auto lw = [&](int l) { return level_dim(w0, l); };
    auto lh = [&](int l) { return level_dim(h0, l); };
    for (int l = 0; l < levels; l++) {
        down[l].resize((size_t)lw(l) * lh(l) * 4);
        for (int y = 0; y < lh(l); y++) for (int x = 0; x < lw(l); x++) {
            if (l == 0) { const FloatImage src = {img.data(), W, H}; store(down[l], lw(l), x, y, down_texel(src, W, H, x, y, lw(l), lh(l), true, set[1], set[0])); }
            else { const HalfLevel src = {down[l - 1].data(), lw(l - 1), lh(l - 1)}; store(down[l], lw(l), x, y, down_texel(src, lw(l - 1), lh(l - 1), x, y, lw(l), lh(l), l == 1, set[1], set[0])); }
        }
    }
    for (int l = levels - 2; l >= 0; l--) {
        up[l].resize((size_t)lw(l) * lh(l) * 4);
        const HalfLevel a = {l == levels - 2 ? down[l + 1].data() : up[l + 1].data(), lw(l + 1), lh(l + 1)}, b = {down[l + 1].data(), lw(l + 1), lh(l + 1)};
        for (int y = 0; y < lh(l); y++) for (int x = 0; x < lw(l); x++) store(up[l], lw(l), x, y, up_texel(a, b, lw(l + 1), lh(l + 1), x, y, lw(l), lh(l)));
    }
    std::vector<float> out((size_t)W * H * 4);
    const HalfLevel up0 = {up[0].data(), w0, h0};
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const V3 r = expand_texel(up0, w0, h0, x, y, W, H);
        float* t = &out[((size_t)y * W + x) * 4]; t[0] = r.x; t[1] = r.y; t[2] = r.z; t[3] = 1.0f;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    const int32_t lv = levels;
    fwrite(&lv, 4, 1, o);
    for (auto& l : down) fwrite(l.data(), 2, l.size(), o);
    for (auto& l : up) fwrite(l.data(), 2, l.size(), o);
    fwrite(out.data(), 4, out.size(), o);
    if (fclose(o) != 0) { perror("close"); return 1; }
    return 0;
}
