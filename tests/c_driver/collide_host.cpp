// collide_host.cpp — idkengine_amd/csrc/collide_sphere.hpp (what k_collide_spheres of kernels_collide.hpp calls per lane) compiled for the HOST and run over a batch of
// spheres: tests/test_collide_ref.py builds this with g++ -ffp-contract=off -fsanitize=address,undefined and compares every record with tests/collide_ref.py's binary32
// restatement bit for bit.  tools/collide_bench.py builds it with -O2 -DCOLLIDE_THREADS -pthread as the CPU baseline.
//   collide_host IN OUT [threads repeats]
// IN:  int32 nodeCount, triCount, descCount, instCount, tlasCount, xformCount, sphereCount, blasCap, tlasCap; idkpt_collide_settings; then GpuBlasNode[nodeCount],
//      triVerts (triCount x 3 x 4 floats), GpuBlasDesc[descCount], GpuBlasInstance[instCount], GpuTlasNode[tlasCount], GpuMeshTransform[xformCount], idkpt_moving_sphere[sphereCount].
// OUT: idkpt_sphere_collision[sphereCount].  Exit status 3: the walk's stack overflowed.  With threads: prints the seconds of the fastest of `repeats` runs.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#ifdef COLLIDE_THREADS
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#endif
#include "../../idkengine_amd/csrc/collide_sphere.hpp"

using namespace collide;

template <class T> static bool read_n(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static void run(const SceneView& s, const idkpt_collide_settings& set, int blasCap, int tlasCap, const idkpt_moving_sphere* in, idkpt_sphere_collision* out, size_t first, size_t end)
{
    std::vector<uint32_t> stk((size_t)blasCap + (size_t)tlasCap + 1);
    Stack stack; stack.p = stk.data(); stack.stride = 1; stack.blasCap = blasCap; stack.tlasCap = tlasCap;
    for (size_t i = first; i < end; i++) out[i] = collide_sphere(s, stack, set, in[i]);
}

int main(int argc, char** argv)
{
    if (argc != 3 && argc != 5) { fprintf(stderr, "usage: collide_host IN OUT [threads repeats]\n"); return 1; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    int32_t h[9]; idkpt_collide_settings set;
    if (fread(h, 4, 9, in) != 9 || fread(&set, sizeof(set), 1, in) != 1) { fprintf(stderr, "short header\n"); return 1; }
    for (int i = 0; i < 9; i++) if (h[i] < 0) { fprintf(stderr, "bad count\n"); return 1; }
    std::vector<F4> nodes, triVerts, tlas, xforms; std::vector<GpuBlasDesc> descs; std::vector<GpuBlasInstance> insts; std::vector<idkpt_moving_sphere> spheres;
    if (!read_n(in, nodes, (size_t)h[0] * 2) || !read_n(in, triVerts, (size_t)h[1] * 3) || !read_n(in, descs, (size_t)h[2]) || !read_n(in, insts, (size_t)h[3]) ||
        !read_n(in, tlas, (size_t)h[4] * 2) || !read_n(in, xforms, (size_t)h[5] * 9) || !read_n(in, spheres, (size_t)h[6])) { fprintf(stderr, "short input\n"); return 1; }
    fclose(in);
    uint32_t overflow = 0u;
    SceneView s;
    s.nodes = nodes.data(); s.triVerts = triVerts.data(); s.descs = descs.data(); s.instances = insts.data(); s.instanceCount = h[3];
    s.tlas = tlas.data(); s.tlasCount = h[4]; s.xforms = xforms.data(); s.overflow = &overflow;
    std::vector<idkpt_sphere_collision> out(spheres.size());
    if (argc == 3) run(s, set, h[7], h[8], spheres.data(), out.data(), 0, spheres.size());
#ifdef COLLIDE_THREADS
    else {
        const int threads = atoi(argv[3]), repeats = atoi(argv[4]);
        if (threads < 1 || threads > 256 || repeats < 1) { fprintf(stderr, "bad threads / repeats\n"); return 1; }
        double best = 1e30;
        for (int r = 0; r < repeats; r++) {
            std::atomic<size_t> next(0);
            const size_t chunk = 16;
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<std::thread> pool;
            for (int t = 0; t < threads; t++) pool.emplace_back([&] { for (;;) { const size_t f = next.fetch_add(chunk); if (f >= spheres.size()) break; run(s, set, h[7], h[8], spheres.data(), out.data(), f, std::min(spheres.size(), f + chunk)); } });
            for (auto& t : pool) t.join();
            best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        printf("%.9f\n", best);
    }
#else
    else { fprintf(stderr, "built without COLLIDE_THREADS\n"); return 1; }
#endif
    if (overflow) { fprintf(stderr, "stack overflow\n"); return 3; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    if (!out.empty()) fwrite(out.data(), sizeof(out[0]), out.size(), o);
    if (fclose(o) != 0) { perror("close"); return 1; }
    return 0;
}
