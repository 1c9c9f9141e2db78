// motion_host.cpp — the per-pixel functions of idkengine_amd/csrc/motion_texel.hpp and reproject_texel.hpp (what k_geom_motion_pack and k_reproject_motion call) compiled
// for the HOST and run the way the kernels run them: tests/test_motion_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares records and
// temporal images with tests/motion_ref.py's binary32 restatement bit for bit.
//   motion_host record IN OUT
//     IN:  int32 N, triCount, vertexCount, xformCount; float o[3]; N * 3 floats d; N floats T, BaryX, BaryY; N uint32 TriangleId, MeshTransformId, Hit;
//          triCount * 4 uint32 (X, Y, Z, MeshId); vertexCount * 3 floats (previous positions); xformCount * 12 floats (PrevModel, three rows of four)
//     OUT: N * 4 floats (the geometry records), then N * 4 floats (the motion records)
//   motion_host texel IN OUT
//     IN:  int32 W, H, extended, moments; float n; float M[16], PrevViewPos[3], PositionTolerance, MaxHistory; then five W * H * 4 float images: cur, g, l, hg, hc
//          (extended = 0: the four-argument texel, l is not used; moments = 1: cur holds (m1, m2, ., .) and reproject_moments_texel runs)
//     OUT: the temporal image (W * H * 4 floats)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../idkengine_amd/csrc/motion_texel.hpp"

using namespace reprojt;

static bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

struct HostFetch {                // k_reproject's MemFetch over host arrays; aborts when asked for a texel outside
    const float* g; const float* c; int W, H;
    void operator()(int x, int y, V4* og, V4* oc) const
    {
        if (x < 0 || x >= W || y < 0 || y >= H) { fprintf(stderr, "fetch outside the image: %d %d\n", x, y); abort(); }
        const size_t i = ((size_t)y * W + x) * 4;
        *og = v4(g[i], g[i + 1], g[i + 2], g[i + 3]); *oc = v4(c[i], c[i + 1], c[i + 2], c[i + 3]);
    }
};

static int run_record(FILE* in, FILE* out)
{
    int32_t hdr[4]; float o[3];
    if (!read_all(in, hdr, 16) || !read_all(in, o, 12)) { fprintf(stderr, "short header\n"); return 1; }
    const int N = hdr[0], nt = hdr[1], nv = hdr[2], nx = hdr[3];
    if (N < 0 || nt < 0 || nv < 0 || nx < 0 || N > (1 << 24) || nt > (1 << 24) || nv > (1 << 24) || nx > (1 << 20)) { fprintf(stderr, "bad header\n"); return 1; }
    std::vector<float> d((size_t)N * 3), T(N), bx(N), by(N), prev((size_t)nv * 3), rows((size_t)nx * 12), geom((size_t)N * 4), motion((size_t)N * 4);
    std::vector<uint32_t> tri(N), xf(N), hit(N), tris((size_t)nt * 4);
    if (!read_all(in, d.data(), (size_t)N * 12) || !read_all(in, T.data(), (size_t)N * 4) || !read_all(in, bx.data(), (size_t)N * 4) || !read_all(in, by.data(), (size_t)N * 4) ||
        !read_all(in, tri.data(), (size_t)N * 4) || !read_all(in, xf.data(), (size_t)N * 4) || !read_all(in, hit.data(), (size_t)N * 4) || !read_all(in, tris.data(), (size_t)nt * 16) ||
        !read_all(in, prev.data(), (size_t)nv * 12) || !read_all(in, rows.data(), (size_t)nx * 48)) { fprintf(stderr, "short input\n"); return 1; }
    for (int i = 0; i < N; i++) {                                              // k_geom_motion_pack's body
        const V4 r = pack_record(o, &d[3 * (size_t)i], T[i], xf[i], hit[i] != 0u);
        V4 m = r;
        if (hit[i] != 0u && motiont::ids_resident(tri[i], (uint32_t)nt, xf[i], (uint32_t)nx)) {
            const uint32_t* v = &tris[4 * (size_t)tri[i]];
            if (motiont::vertices_resident(v[0], v[1], v[2], (uint32_t)nv)) {
                const float* x = &rows[12 * (size_t)xf[i]];
                m = motiont::prev_record(bx[i], by[i], &prev[3 * (size_t)v[0]], &prev[3 * (size_t)v[1]], &prev[3 * (size_t)v[2]], v4(x[0], x[1], x[2], x[3]), v4(x[4], x[5], x[6], x[7]), v4(x[8], x[9], x[10], x[11]), xf[i]);
            }
        }
        const size_t k = 4 * (size_t)i;
        geom[k] = r.x; geom[k + 1] = r.y; geom[k + 2] = r.z; geom[k + 3] = r.w;
        motion[k] = m.x; motion[k + 1] = m.y; motion[k + 2] = m.z; motion[k + 3] = m.w;
    }
    fwrite(geom.data(), 4, geom.size(), out); fwrite(motion.data(), 4, motion.size(), out);
    return 0;
}

static int run_texel(FILE* in, FILE* out)
{
    int32_t hdr[4]; float n, M[16], pos[3], par[2];
    if (!read_all(in, hdr, 16) || !read_all(in, &n, 4) || !read_all(in, M, 64) || !read_all(in, pos, 12) || !read_all(in, par, 8)) { fprintf(stderr, "short header\n"); return 1; }
    const int W = hdr[0], H = hdr[1]; const bool extended = hdr[2] != 0, moments = hdr[3] != 0;
    if (W < 1 || H < 1 || W > 4096 || H > 4096) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t N = (size_t)W * H;
    std::vector<float> cur(N * 4), g(N * 4), l(N * 4), hg(N * 4), hc(N * 4), res(N * 4);
    if (!read_all(in, cur.data(), N * 16) || !read_all(in, g.data(), N * 16) || !read_all(in, l.data(), N * 16) || !read_all(in, hg.data(), N * 16) || !read_all(in, hc.data(), N * 16)) { fprintf(stderr, "short images\n"); return 1; }
    Params p;
    p.W = W; p.H = H; memcpy(p.M, M, 64); memcpy(p.prevPos, pos, 12);
    p.tol2 = par[0] * par[0]; p.maxHistory = par[1]; p.n = n;          // (host_reproject.hpp: the product once per call)
    const HostFetch f = {hg.data(), hc.data(), W, H};
    for (size_t i = 0; i < N * 4; i += 4) {
        const V4 c = v4(cur[i], cur[i + 1], cur[i + 2], cur[i + 3]), rg = v4(g[i], g[i + 1], g[i + 2], g[i + 3]), rl = v4(l[i], l[i + 1], l[i + 2], l[i + 3]);
        V4 o;
        if (moments) o = extended ? reproject_moments_texel(f, p, c.x, c.y, rg, rl) : reproject_moments_texel(f, p, c.x, c.y, rg);
        else o = extended ? reproject_texel(f, p, c, rg, rl) : reproject_texel(f, p, c, rg);
        res[i] = o.x; res[i + 1] = o.y; res[i + 2] = o.z; res[i + 3] = o.w;
    }
    fwrite(res.data(), 4, res.size(), out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: motion_host record|texel IN OUT\n"); return 1; }
    FILE* in = fopen(argv[2], "rb");
    if (!in) { perror(argv[2]); return 1; }
    FILE* out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 1; }
    int rc = 1;
    if (!strcmp(argv[1], "record")) rc = run_record(in, out);
    else if (!strcmp(argv[1], "texel")) rc = run_texel(in, out);
    else fprintf(stderr, "unknown mode %s\n", argv[1]);
    fclose(in);
    if (fclose(out) != 0) { perror("close"); return 1; }
    return rc;
}
