// denoise_temporal_host.cpp — the per-pixel functions of idkengine_amd/csrc/denoise_temporal_texel.hpp and reproject_texel.hpp's reproject_moments_texel (what the device
// kernels k_temporal_state and k_reproject_moments call) compiled for the HOST and run over a whole frame the way host_denoise_temporal.hpp and host_reproject.hpp run the
// launches: tests/test_denoise_temporal_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares the images with
// tests/denoise_temporal_ref.py's binary32 restatement bit for bit.
//   denoise_temporal_host filter|moments IN OUT
// filter  IN: int32 W, H, Iterations, DemodulateAlbedo; float LumaSigma, VarianceEpsilon, AlbedoSigma, NormalSigma, SpatialBelow; then the temporal image, the temporal
//             moments, Albedo, Normal: W * H * 4 floats each.  OUT: W * H * 4 floats (rgb, 1.0).
// moments IN: int32 W, H, start; float n, PrevProjView[16], PrevViewPos[3], PositionTolerance, MaxHistory; then the moments image, the geometry image, the history slot's
//             geometry and temporal moments images: W * H * 4 floats each.  OUT: W * H * 4 floats (M1, M2, 0, cnt).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/denoise_temporal_texel.hpp"
#include "denoise_state_host.hpp"
#include "../../idkengine_amd/csrc/reproject_texel.hpp"

using denoiset::V3;
using denoiset::v3;
using denoisevt::State;

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

struct MomentsFetch {                    // as kernels_denoise_temporal.hpp LdsFetch: (M1, M2, cnt) are channels x, y, w.  Aborts on a texel outside the image
    const float* m; const float* a; const float* n; int W, H;
    void operator()(int x, int y, V3* om, V3* oa, V3* on) const
    {
        if (x < 0 || x >= W || y < 0 || y >= H) { fprintf(stderr, "fetch outside the image\n"); abort(); }
        const size_t i = ((size_t)y * (size_t)W + (size_t)x) * 4;
        *om = v3(m[i], m[i + 1], m[i + 3]); *oa = v3(a[i], a[i + 1], a[i + 2]); *on = v3(n[i], n[i + 1], n[i + 2]);
    }
};

struct HistoryFetch {                    // as kernels_reproject.hpp MemFetch
    const float* g; const float* c; int W, H;
    void operator()(int x, int y, reprojt::V4* og, reprojt::V4* oc) const
    {
        if (x < 0 || x >= W || y < 0 || y >= H) { fprintf(stderr, "fetch outside the image\n"); abort(); }
        const size_t i = ((size_t)y * W + x) * 4;
        *og = reprojt::v4(g[i], g[i + 1], g[i + 2], g[i + 3]); *oc = reprojt::v4(c[i], c[i + 1], c[i + 2], c[i + 3]);
    }
};

static int run_filter(FILE* in, FILE* out)
{
    int32_t hdr[4]; float sig[5];
    if (!read_all(in, hdr, 16) || !read_all(in, sig, 20)) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1], iterations = hdr[2], demod = hdr[3];
    if (W < 1 || H < 1 || W > 4096 || H > 4096 || iterations < 1 || iterations > denoiset::MAX_ITERATIONS || (demod != 0 && demod != 1)) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t N = (size_t)W * H * 4;
    std::vector<float> temporal(N), moments(N), albedo(N), normal(N);
    if (!read_all(in, temporal.data(), N * 4) || !read_all(in, moments.data(), N * 4) || !read_all(in, albedo.data(), N * 4) || !read_all(in, normal.data(), N * 4)) { fprintf(stderr, "short images\n"); return 1; }
    const float ls2 = sig[0] * sig[0], eps = sig[1], invA = denoiset::inv_sigma2(sig[2], 0), invN = denoiset::inv_sigma2(sig[3], 0), spatialBelow = sig[4];

    // the pre-pass into ping[1], iteration i into ping[i & 1] (denoise_state_host.hpp)
    std::vector<float> ping[2] = {std::vector<float>(N), std::vector<float>(N)};
    const MomentsFetch mf = {moments.data(), albedo.data(), normal.data(), W, H};
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const size_t k = ((size_t)y * W + x) * 4;
        const State st = denoisett::temporal_state(mf, W, H, x, y, v3(temporal[k], temporal[k + 1], temporal[k + 2]), spatialBelow, invA, invN, demod != 0);
        ping[1][k] = st.c.x; ping[1][k + 1] = st.c.y; ping[1][k + 2] = st.c.z; ping[1][k + 3] = st.v;
    }
    const float* src = variance_iterations(ping[1].data(), ping, albedo.data(), normal.data(), W, H, iterations, demod, ls2, eps, invA, invN);
    fwrite(src, 4, N, out);
    return 0;
}

static int run_moments(FILE* in, FILE* out)
{
    int32_t hdr[3]; float n, M[16], pos[3], par[2];
    if (!read_all(in, hdr, 12) || !read_all(in, &n, 4) || !read_all(in, M, 64) || !read_all(in, pos, 12) || !read_all(in, par, 8)) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1], start = hdr[2];
    if (W < 1 || H < 1 || W > 4096 || H > 4096) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t N = (size_t)W * H;
    std::vector<float> mom(N * 4), g(N * 4), hg(N * 4), hm(N * 4), res(N * 4);
    if (!read_all(in, mom.data(), N * 16) || !read_all(in, g.data(), N * 16) || !read_all(in, hg.data(), N * 16) || !read_all(in, hm.data(), N * 16)) { fprintf(stderr, "short images\n"); return 1; }
    reprojt::Params p;
    p.W = W; p.H = H; memcpy(p.M, M, 64); memcpy(p.prevPos, pos, 12);
    p.tol2 = par[0] * par[0]; p.maxHistory = par[1]; p.n = n;          // (host_reproject.hpp: the product once per call)
    const HistoryFetch f = {hg.data(), hm.data(), W, H};
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const size_t i = ((size_t)y * W + x) * 4;
        reprojt::V4 o = reprojt::v4(mom[i], mom[i + 1], 0.0f, n);      // (k_reproject_moments: the history start)
        if (!start) o = reprojt::reproject_moments_texel(f, p, mom[i], mom[i + 1], reprojt::v4(g[i], g[i + 1], g[i + 2], g[i + 3]));
        res[i] = o.x; res[i + 1] = o.y; res[i + 2] = o.z; res[i + 3] = o.w;
    }
    fwrite(res.data(), 4, res.size(), out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: denoise_temporal_host filter|moments IN OUT\n"); return 1; }
    FILE* in = fopen(argv[2], "rb");
    if (!in) { perror(argv[2]); return 1; }
    FILE* out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 1; }
    int rc = 1;
    if (!strcmp(argv[1], "filter")) rc = run_filter(in, out);
    else if (!strcmp(argv[1], "moments")) rc = run_moments(in, out);
    else fprintf(stderr, "unknown mode %s\n", argv[1]);
    fclose(in);
    if (fclose(out) != 0) { perror("close"); return 1; }
    return rc;
}
