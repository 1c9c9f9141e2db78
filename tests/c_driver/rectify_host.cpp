// rectify_host.cpp — the per-pixel function of idkengine_amd/csrc/rectify_texel.hpp (what k_rectify calls) compiled for the HOST and run the way the kernel runs it:
// tests/test_rectify_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares the image with tests/rectify_ref.py's binary32 restatement
// bit for bit.
//   rectify_host IN OUT
//     IN:  int32 W, H, Radius; float ZLow, ZHigh, Epsilon; then three W * H * 4 float images: t (temporal), f (fast temporal), g (geometry)
//     OUT: the rectified temporal image (W * H * 4 floats), then W * H uint32: 1 where the blend branch ran
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/rectify_texel.hpp"

using namespace rectt;

static bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

struct HostFetch {                // k_rectify's staged difference records over host arrays; aborts when asked for a texel outside
    const float* t; const float* f; const float* g; int W, H;
    V4 at(const float* a, size_t i) const { return v4(a[i], a[i + 1], a[i + 2], a[i + 3]); }
    V4 operator()(int x, int y) const
    {
        if (x < 0 || x >= W || y < 0 || y >= H) { fprintf(stderr, "fetch outside the image: %d %d\n", x, y); abort(); }
        const size_t i = ((size_t)y * W + x) * 4;
        return difference(at(f, i), at(t, i), g[i + 3]);
    }
};

template <int R>
static void run(const HostFetch& fetch, const Params& p, std::vector<float>& res, std::vector<uint32_t>& blended)
{
    for (int y = 0; y < p.H; y++)
        for (int x = 0; x < p.W; x++) {
            const size_t k = (size_t)y * p.W + x, i = k * 4;
            const Texel r = rectify_texel<R>(fetch, p, x, y, fetch.at(fetch.f, i), fetch.at(fetch.t, i));
            res[i] = r.out.x; res[i + 1] = r.out.y; res[i + 2] = r.out.z; res[i + 3] = r.out.w;
            blended[k] = r.blended ? 1u : 0u;
        }
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: rectify_host IN OUT\n"); return 1; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    int32_t hdr[3]; float par[3];
    if (!read_all(in, hdr, 12) || !read_all(in, par, 12)) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1], R = hdr[2];
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || R < 1 || R > MAX_RADIUS) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t N = (size_t)W * H;
    std::vector<float> t(N * 4), f(N * 4), g(N * 4), res(N * 4);
    std::vector<uint32_t> blended(N);
    if (!read_all(in, t.data(), N * 16) || !read_all(in, f.data(), N * 16) || !read_all(in, g.data(), N * 16)) { fprintf(stderr, "short images\n"); return 1; }
    fclose(in);
    Params p;
    p.W = W; p.H = H;
    p.eps2 = par[2] * par[2]; p.lo2 = par[0] * par[0]; p.span = par[1] * par[1] - p.lo2;      // (host_rectify.hpp: once per call)
    const HostFetch fetch = {t.data(), f.data(), g.data(), W, H};
    if (R == 1) run<1>(fetch, p, res, blended);
    else if (R == 2) run<2>(fetch, p, res, blended);
    else run<3>(fetch, p, res, blended);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 1; }
    fwrite(res.data(), 4, res.size(), out); fwrite(blended.data(), 4, blended.size(), out);
    if (fclose(out) != 0) { perror("close"); return 1; }
    return 0;
}
