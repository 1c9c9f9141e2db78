// reconstruct_host.cpp — the per-pixel function of idkengine_amd/csrc/reconstruct_texel.hpp (what k_reconstruct calls) compiled for the HOST and run over a frame:
// tests/test_reconstruct_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares the image with tests/reconstruct_ref.py's binary32
// restatement bit for bit.  Unlike the kernel it reads the input image and writes ANOTHER one, so it states what the in-place kernel must equal.
//   reconstruct_host IN OUT
//     IN:  int32 W, H, Radius, Stride; float FillBelow, AlbedoSigma, NormalSigma; then four W * H * 4 float images: t (temporal), g (geometry), a (albedo), n (normal)
//     OUT: the reconstructed temporal image (W * H * 4 floats), then W * H uint32: 1 where the pixel was written
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/reconstruct_texel.hpp"

using namespace recont;

static bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

struct HostFetch {                // k_reconstruct's fetches over host arrays; aborts when asked for a texel outside
    const float* t; const float* g; const float* a; const float* n; int W, H;
    size_t at(int x, int y) const
    {
        if (x < 0 || x >= W || y < 0 || y >= H) { fprintf(stderr, "fetch outside the image: %d %d\n", x, y); abort(); }
        return ((size_t)y * W + x) * 4;
    }
    void history(int x, int y, V4* ot, uint32_t* oid) const { const size_t i = at(x, y); *ot = v4(t[i], t[i + 1], t[i + 2], t[i + 3]); *oid = bits_of(g[i + 3]); }
    void guides(int x, int y, V3* oa, V3* on) const { const size_t i = at(x, y); *oa = denoiset::v3(a[i], a[i + 1], a[i + 2]); *on = denoiset::v3(n[i], n[i + 1], n[i + 2]); }
};

template <int R>
static void run(const HostFetch& fetch, const Params& p, std::vector<float>& res, std::vector<uint32_t>& written)
{
    for (int y = 0; y < p.H; y++)
        for (int x = 0; x < p.W; x++) {
            const size_t k = (size_t)y * p.W + x, i = k * 4;
            const Texel r = reconstruct_texel<R>(fetch, p, x, y);
            res[i] = r.out.x; res[i + 1] = r.out.y; res[i + 2] = r.out.z; res[i + 3] = r.out.w;
            written[k] = r.written ? 1u : 0u;
        }
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: reconstruct_host IN OUT\n"); return 1; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    int32_t hdr[4]; float par[3];
    if (!read_all(in, hdr, 16) || !read_all(in, par, 12)) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1], R = hdr[2], stride = hdr[3];
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || R < 1 || R > MAX_RADIUS || stride < 1 || stride > MAX_STRIDE) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t N = (size_t)W * H;
    std::vector<float> t(N * 4), g(N * 4), a(N * 4), n(N * 4), res(N * 4);
    std::vector<uint32_t> written(N);
    if (!read_all(in, t.data(), N * 16) || !read_all(in, g.data(), N * 16) || !read_all(in, a.data(), N * 16) || !read_all(in, n.data(), N * 16)) { fprintf(stderr, "short images\n"); return 1; }
    fclose(in);
    Params p;
    p.W = W; p.H = H; p.stride = stride; p.fillBelow = par[0];
    p.invA = denoiset::inv_sigma2(par[1], 0); p.invN = denoiset::inv_sigma2(par[2], 0);          // (host_reconstruct.hpp: once per call)
    const HostFetch fetch = {t.data(), g.data(), a.data(), n.data(), W, H};
    if (R == 1) run<1>(fetch, p, res, written);
    else if (R == 2) run<2>(fetch, p, res, written);
    else run<3>(fetch, p, res, written);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 1; }
    fwrite(res.data(), 4, res.size(), out); fwrite(written.data(), 4, written.size(), out);
    if (fclose(out) != 0) { perror("close"); return 1; }
    return 0;
}
