// reproject_host.cpp — the per-pixel functions of idkengine_amd/csrc/reproject_texel.hpp (what k_geom_pack and k_reproject call) compiled for the HOST and run over a whole
// frame the way the kernels run them: tests/test_reproject_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares records and temporal
// images with tests/reproject_ref.py's binary32 restatement bit for bit.  A third mode generates centre rays with the ORACLE's GetWorldSpaceDirection (oracle/ref_math.h):
// the rays tests/test_gpu_reproject.py hands to idkptTraceRays, and what the restatement's own ray generation is held to.
//   reproject_host texel IN OUT
//     IN:  int32 W, H; float n; float M[16], PrevViewPos[3], PositionTolerance, MaxHistory; then four W * H * 4 float images: cur, g, hg, hc
//     OUT: the temporal image (W * H * 4 floats)
//   reproject_host pack IN OUT
//     IN:  int32 N; float o[3]; N * 3 floats d; N floats T; N uint32 MeshTransformId; N uint32 Hit
//     OUT: N * 4 floats
//   reproject_host rays IN OUT
//     IN:  int32 W, H; float InvProjection[16], InvView[16]
//     OUT: float o[3]; W * H * 3 floats d, row-major
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/reproject_texel.hpp"
#include "../../oracle/ref_math.h"

using namespace reprojt;

static bool read_all(FILE* f, void* dst, size_t bytes) { return fread(dst, 1, bytes, f) == bytes; }

struct HostFetch {                // k_reproject's MemFetch over host arrays; asserts what the kernel relies on: never called for a texel outside
    const float* g; const float* c; int W, H;
    void operator()(int x, int y, V4* og, V4* oc) const
    {
        if (x < 0 || x >= W || y < 0 || y >= H) { fprintf(stderr, "fetch outside the image: %d %d\n", x, y); abort(); }
        const size_t i = ((size_t)y * W + x) * 4;
        *og = v4(g[i], g[i + 1], g[i + 2], g[i + 3]); *oc = v4(c[i], c[i + 1], c[i + 2], c[i + 3]);
    }
};

static int run_texel(FILE* in, FILE* out)
{
    int32_t hdr[2]; float n, M[16], pos[3], par[2];
    if (!read_all(in, hdr, 8) || !read_all(in, &n, 4) || !read_all(in, M, 64) || !read_all(in, pos, 12) || !read_all(in, par, 8)) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1];
    if (W < 1 || H < 1 || W > 4096 || H > 4096) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t N = (size_t)W * H;
    std::vector<float> cur(N * 4), g(N * 4), hg(N * 4), hc(N * 4), res(N * 4);
    if (!read_all(in, cur.data(), N * 16) || !read_all(in, g.data(), N * 16) || !read_all(in, hg.data(), N * 16) || !read_all(in, hc.data(), N * 16)) { fprintf(stderr, "short images\n"); return 1; }
    Params p;
    p.W = W; p.H = H; memcpy(p.M, M, 64); memcpy(p.prevPos, pos, 12);
    p.tol2 = par[0] * par[0]; p.maxHistory = par[1]; p.n = n;          // (host_reproject.hpp: the product once per call)
    const HostFetch f = {hg.data(), hc.data(), W, H};
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const size_t i = ((size_t)y * W + x) * 4;
        const V4 o = reproject_texel(f, p, v4(cur[i], cur[i + 1], cur[i + 2], cur[i + 3]), v4(g[i], g[i + 1], g[i + 2], g[i + 3]));
        res[i] = o.x; res[i + 1] = o.y; res[i + 2] = o.z; res[i + 3] = o.w;
    }
    fwrite(res.data(), 4, res.size(), out);
    return 0;
}

static int run_pack(FILE* in, FILE* out)
{
    int32_t N; float o[3];
    if (!read_all(in, &N, 4) || !read_all(in, o, 12) || N < 0 || N > (1 << 24)) { fprintf(stderr, "bad header\n"); return 1; }
    std::vector<float> d((size_t)N * 3), T(N), res((size_t)N * 4); std::vector<uint32_t> id(N), hit(N);
    if (!read_all(in, d.data(), (size_t)N * 12) || !read_all(in, T.data(), (size_t)N * 4) || !read_all(in, id.data(), (size_t)N * 4) || !read_all(in, hit.data(), (size_t)N * 4)) { fprintf(stderr, "short input\n"); return 1; }
    for (int i = 0; i < N; i++) {
        const V4 r = pack_record(o, &d[3 * (size_t)i], T[i], id[i], hit[i] != 0u);
        res[4 * (size_t)i] = r.x; res[4 * (size_t)i + 1] = r.y; res[4 * (size_t)i + 2] = r.z; res[4 * (size_t)i + 3] = r.w;
    }
    fwrite(res.data(), 4, res.size(), out);
    return 0;
}

static int run_rays(FILE* in, FILE* out)
{
    int32_t hdr[2]; float ip[16], iv[16];
    if (!read_all(in, hdr, 8) || !read_all(in, ip, 64) || !read_all(in, iv, 64)) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1];
    if (W < 1 || H < 1 || W > 4096 || H > 4096) { fprintf(stderr, "bad header\n"); return 1; }
    std::vector<float> d((size_t)W * H * 3);
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const ref::v2 ndc = {((float)x + 0.5f) / (float)W * 2.0f - 1.0f, ((float)y + 0.5f) / (float)H * 2.0f - 1.0f};
        const ref::v3 r = ref::GetWorldSpaceDirection(ip, iv, ndc);
        const size_t i = ((size_t)y * W + x) * 3;
        d[i] = r.x; d[i + 1] = r.y; d[i + 2] = r.z;
    }
    fwrite(&iv[12], 4, 3, out); fwrite(d.data(), 4, d.size(), out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: reproject_host texel|pack|rays IN OUT\n"); return 1; }
    FILE* in = fopen(argv[2], "rb");
    if (!in) { perror(argv[2]); return 1; }
    FILE* out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 1; }
    int rc = 1;
    if (!strcmp(argv[1], "texel")) rc = run_texel(in, out);
    else if (!strcmp(argv[1], "pack")) rc = run_pack(in, out);
    else if (!strcmp(argv[1], "rays")) rc = run_rays(in, out);
    else fprintf(stderr, "unknown mode %s\n", argv[1]);
    fclose(in);
    if (fclose(out) != 0) { perror("close"); return 1; }
    return rc;
}
