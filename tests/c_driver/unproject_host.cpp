// unproject_host.cpp — the per-texel functions of idkengine_amd/csrc/unproject_texel.hpp (what the device kernels of kernels_unproject.hpp call) compiled for the HOST and
// run over a whole panorama: tests/test_unproject_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares with tests/unproject_ref.py.
//   unproject_host IN OUT
// IN:  int32 W, H, channels, S, nUV, nStore; W * H * channels floats (the panorama); nUV pairs of floats (u, v); nStore floats.
// OUT: W * H * 4 uint16 (the packed panorama); 6 * S * S * 4 floats (what imageStore receives); 6 * S * S * 4 uint16 (the cube's halves);
//      per (u, v): int32 x0, x1, y0, y1 and float ax, ay (linear_taps on W and on H); nStore uint16 (f32_to_f16_rtz of the given floats).
// Additionally checks f32_to_f16_rne against a list of values whose halves are known (exit status 2 on a mismatch).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/unproject_texel.hpp"

using namespace unprojt;

static int self_check()
{
    struct { float f; uint16_t h; } k[] = {
        {0.0f, 0x0000}, {-0.0f, 0x8000}, {1.0f, 0x3C00}, {1.0009765625f, 0x3C01}, {1.00048828125f, 0x3C00} /* a tie: to even */, {1.00146484375f, 0x3C02} /* a tie: to even, up */,
        {-1.00146484375f, 0xBC02}, {1.0004884f, 0x3C01} /* just above a tie */, {1.9995118f, 0x4000} /* the carry moves into the exponent */, {65504.0f, 0x7BFF}, {65519.996f, 0x7BFF},
        {65520.0f, 0x7BFF} /* the nearest half would be infinite: saturates */, {3.0e38f, 0x7BFF}, {-70000.0f, 0xFBFF}, {6.103515625e-5f, 0x0400} /* the smallest normal half */,
        {6.1e-5f, 0x03FF}, {6.1006e-5f, 0x0400} /* rounds up into the normals */, {5.9604644775390625e-8f, 0x0001}, {2.98023223876953125e-8f, 0x0000} /* 2^-25: a tie, to the even zero */,
        {2.9802326e-8f, 0x0001} /* just above it */, {8.94069671630859375e-8f, 0x0002} /* 1.5 * 2^-24: a tie, to even */, {1e-30f, 0x0000}, {-1.5e-7f, 0x8003}, {0.04045f, 0x292D},
    };
    for (auto& c : k) if (f32_to_f16_rne(c.f) != c.h) { fprintf(stderr, "f32_to_f16_rne(%a) = %04x, want %04x\n", c.f, f32_to_f16_rne(c.f), c.h); return 2; }
    for (uint32_t h = 0; h < 0x10000u; h++) {                 // every finite half survives the round trip under both rules
        if (((h >> 10) & 31u) == 31u) continue;
        if (f32_to_f16_rne(f16_to_f32((uint16_t)h)) != h || f32_to_f16_rtz(f16_to_f32((uint16_t)h)) != h) { fprintf(stderr, "round trip of half %04x\n", h); return 2; }
    }
    if (wrap_repeat(-1, 16) != 15 || wrap_repeat(16, 16) != 0 || wrap_repeat(-17, 16) != 15 || wrap_repeat(5, 16) != 5 || wrap_repeat(0, 1) != 0 || wrap_repeat(-3, 1) != 0) { fprintf(stderr, "wrap_repeat\n"); return 2; }
    return 0;
}

int main(int argc, char** argv)
{
    if (self_check()) return 2;
    if (argc != 3) { fprintf(stderr, "usage: unproject_host IN OUT\n"); return 1; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    int32_t hdr[6];
    if (fread(hdr, 4, 6, in) != 6) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1], ch = hdr[2], S = hdr[3], nUV = hdr[4], nStore = hdr[5];
    if (W < 1 || H < 1 || W > 16384 || H > 8192 || (ch != 3 && ch != 4) || S < 1 || S > 4096 || nUV < 0 || nStore < 0) { fprintf(stderr, "bad sizes\n"); return 1; }
    std::vector<float> img((size_t)W * H * ch), uv((size_t)nUV * 2), st((size_t)nStore);
    if (fread(img.data(), 4, img.size(), in) != img.size() || fread(uv.data(), 4, uv.size(), in) != uv.size() || fread(st.data(), 4, st.size(), in) != st.size()) { fprintf(stderr, "short input\n"); return 1; }
    fclose(in);

    std::vector<uint16_t> pano((size_t)W * H * 4);
    for (size_t t = 0; t < (size_t)W * H; t++) {
        const float* s = &img[t * ch];
        const H4 h = pack_texel(s[0], s[1], s[2], ch == 4 ? s[3] : 1.0f);
        pano[t * 4] = h.x; pano[t * 4 + 1] = h.y; pano[t * 4 + 2] = h.z; pano[t * 4 + 3] = h.w;
    }
    const HalfImage src = {pano.data(), W};
    std::vector<float> val((size_t)6 * S * S * 4);
    std::vector<uint16_t> cube((size_t)6 * S * S * 4);
    for (int f = 0; f < 6; f++) for (int y = 0; y < S; y++) for (int x = 0; x < S; x++) {
        const size_t o = (((size_t)f * S + y) * S + x) * 4;
        const V4 v = unproject_value(src, W, H, x, y, f, S);
        const H4 h = store_texel(v);
        val[o] = v.x; val[o + 1] = v.y; val[o + 2] = v.z; val[o + 3] = v.w;
        cube[o] = h.x; cube[o + 1] = h.y; cube[o + 2] = h.z; cube[o + 3] = h.w;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    fwrite(pano.data(), 2, pano.size(), o);
    fwrite(val.data(), 4, val.size(), o);
    fwrite(cube.data(), 2, cube.size(), o);
    for (int k = 0; k < nUV; k++) {
        int32_t idx[4]; float a[2];
        linear_taps(uv[(size_t)k * 2], W, &idx[0], &idx[1], &a[0]);
        linear_taps(uv[(size_t)k * 2 + 1], H, &idx[2], &idx[3], &a[1]);
        fwrite(idx, 4, 4, o); fwrite(a, 4, 2, o);
    }
    for (int k = 0; k < nStore; k++) { const uint16_t h = f32_to_f16_rtz(st[k]); fwrite(&h, 2, 1, o); }
    if (fclose(o) != 0) { perror("close"); return 1; }
    return 0;
}
