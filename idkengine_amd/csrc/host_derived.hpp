// host_derived.hpp — the derivations of dev_ctx::derived (DerivedScene, host_context.hpp): each *_prepare (re-)derives what is stale of one structure, stream-ordered in front of the
// batch that is about to be launched, and marks it; what makes it stale again is derived_scene.hpp's table.  With one scene version every update launches the queued samples first.
// Part of the single translation unit idkpt.hip (included there, in this order).
#pragma once
using namespace derived;
// totals of the optional walks since idkptResetStats (idkpt_stats.Wide*, InstTlasFlaggedRays, Packet*): sixteen 64-bit words ([0..3] wide, [4] own TLAS, [8..13] packets), zeroed when first needed
#define TOTALS_BYTES 128
static int totals_ensure(dev_ctx* ctx) { if (!ctx->wtotals.p) { HIPC(ctx->wtotals.ensure(TOTALS_BYTES)); HIPC(hipMemsetAsync(ctx->wtotals.p, 0, TOTALS_BYTES, ctx->stream)); } return IDKPT_OK; }
// LDS rows behind the BLAS stack: the own TLAS's stack, or an instance mask of 32 x that many bits.  A tree over n leaves is never deeper than n; once k_tlas_build has reported the depth of the
// tree it built (host-mapped, possibly one rebuild stale: a ray that needs more rows than it gets is flagged and traced by the exact loop) the rows are that depth, and what the mask needs
static int inst_tlas_rows(const dev_ctx* ctx)
{
    if (ctx->derived.itlasDepth > 0 && ctx->derived.holds(TLAS_BUILT)) return std::min(TLAS_STACK_SIZE, std::max((ctx->instanceCount + 31) / 32, ctx->derived.itlasDepth));
    return std::min(TLAS_STACK_SIZE, std::max(1, ctx->instanceCount));
}

// ---- wide nodes (kernels_wide.hpp): the children lists after an upload / a node patch (k_wide_topo, one workgroup per BLAS), box bytes and leaf records after anything that
// moved boxes or positions (k_wide_fill)
static int wide_prepare(dev_ctx* ctx)
{
    DerivedScene& d = ctx->derived;
    if (d.holds(WIDE_TOPO) && d.holds(WIDE_FILL)) return IDKPT_OK;
    { int rc = totals_ensure(ctx); if (rc) return rc; }
    const size_t nb = ctx->hDescs.size();
    hipStream_t st = ctx->stream;
    const float4* nodes = (const float4*)vb_ptr(ctx, VB_NODES, ctx->vcur[VB_NODES]);
    const float4* triVerts = (const float4*)vb_ptr(ctx, VB_TRIVERTS, ctx->vcur[VB_TRIVERTS]);
    if (!d.holds(WIDE_TOPO)) {
        d.wNodeOff.assign(nb + 1, 0u); d.wLeafOff.assign(nb + 1, 0u);
        for (size_t b = 0; b < nb; b++) {
            const GpuBlasDesc& bd = ctx->hDescs[b];
            const uint32_t pairs = (uint32_t)std::max(0, bd.NodeCount) / 2u + 1u, leavesMax = pairs + 1u;                       // a wide node stands for at least one pair; a tree of L leaves has L - 1 internal nodes
            d.wNodeOff[b + 1] = d.wNodeOff[b] + pairs;
            d.wLeafOff[b + 1] = d.wLeafOff[b] + 5u * leavesMax + 3u * (uint32_t)std::max(0, bd.TriangleCount) + 4u;   // 2 + 3 per leaf-range triangle (a leaf pair may share one triangle)
        }
        HIPC(d.wnodes.ensure((size_t)d.wNodeOff[nb] * 64 + 64)); HIPC(d.wids.ensure((size_t)d.wNodeOff[nb] * 16 + 16)); HIPC(d.wpair.ensure((size_t)d.wNodeOff[nb] * 4 + 16));
        HIPC(d.wleaf.ensure((size_t)d.wLeafOff[nb] * 16 + 80)); HIPC(d.wcounts.ensure(nb * 8 + 8));
        for (size_t b = 0; b < nb; b++) {
            const GpuBlasDesc& bd = ctx->hDescs[b];
            hipLaunchKernelGGL(k_wide_topo, dim3(1), dim3(WIDE_TOPO_THREADS), 0, st, nodes + 2 * (size_t)bd.NodeOffset, (uint32_t)bd.NodeCount, d.wpair.as<uint32_t>() + d.wNodeOff[b],
                               d.wids.as<uint4>() + d.wNodeOff[b], d.wnodes.as<uint4>() + 4 * (size_t)d.wNodeOff[b], d.wcounts.as<uint32_t>() + 2 * b);
        }
        HIPC(hipGetLastError());
        d.mark(WIDE_TOPO); d.rederiving(WIDE_TOPO);   // (new children lists: boxes and leaf records are filled below)
    }
    for (size_t b = 0; b < nb; b++) {
        const GpuBlasDesc& bd = ctx->hDescs[b];
        const uint32_t pairs = d.wNodeOff[b + 1] - d.wNodeOff[b];
        hipLaunchKernelGGL(k_wide_fill, dim3((pairs + 255) / 256), dim3(256), 0, st, nodes + 2 * (size_t)bd.NodeOffset, triVerts + 3 * (size_t)bd.TriangleOffset, (const uint4*)(d.wids.as<uint4>() + d.wNodeOff[b]),
                           d.wnodes.as<uint4>() + 4 * (size_t)d.wNodeOff[b], d.wleaf.as<float4>() + d.wLeafOff[b], (const uint32_t*)(d.wcounts.as<uint32_t>() + 2 * b));
    }
    HIPC(hipGetLastError());
    d.mark(WIDE_FILL);
    return IDKPT_OK;
}

// ---- instance records (DScene::instRec, k_inst_records) for the walk through the library's own TLAS: stream-ordered in front of the launch that reads them -----------
static int inst_records_prepare(dev_ctx* ctx)
{
    DerivedScene& d = ctx->derived;
    if (d.holds(INST_REC) || ctx->instanceCount < 2 || ctx->verSlots != 1) return IDKPT_OK;
    HIPC(d.instRec.ensure((size_t)ctx->instanceCount * 96));
    hipLaunchKernelGGL(k_inst_records, dim3((ctx->instanceCount + 255) / 256), dim3(256), 0, ctx->stream, (const float4*)vb_ptr(ctx, VB_NODES, ctx->vcur[VB_NODES]), ctx->descs.as<GpuBlasDesc>(),
                       ctx->instances.as<GpuBlasInstance>(), (const float4*)vb_ptr(ctx, VB_XFORMS, ctx->vcur[VB_XFORMS]), ctx->instanceCount, d.instRec.as<float4>());
    HIPC(hipGetLastError());
    d.mark(INST_REC);
    return IDKPT_OK;
}

// ---- the per-triangle marks "not contained in its leaf box" (k_mark_triangles) of the walks that re-order a ray's candidates (k_trace_inst, k_trace_packet): derived on the
// device before the first launch that wants them and after everything that moved boxes or positions (one scene version only)
static int chunks_ensure(dev_ctx* ctx)
{
    DerivedScene& d = ctx->derived;
    if (d.holds(CHUNKS)) return IDKPT_OK;   // the flattened (BLAS, chunk of 256 nodes) table: once per upload
    hipStream_t st = ctx->stream;
    std::vector<uint32_t> tab;
    for (size_t b = 0; b < ctx->hDescs.size(); b++) for (int first = 0; first < ctx->hDescs[b].NodeCount; first += 256) { tab.push_back((uint32_t)b); tab.push_back((uint32_t)first); }
    d.ichunkCount = (uint32_t)(tab.size() / 2);
    HIPC(d.ichunks.ensure(tab.size() * 4 + 8));
    if (!tab.empty()) { HIPC(hipMemcpyAsync(d.ichunks.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st)); HIPC(hipStreamSynchronize(st)); }   // (tab is a stack vector)
    d.mark(CHUNKS);
    return IDKPT_OK;
}
static int marks_prepare(dev_ctx* ctx)
{
    DerivedScene& d = ctx->derived;
    if (d.holds(MARKS)) return IDKPT_OK;
    hipStream_t st = ctx->stream;
    { int rc = chunks_ensure(ctx); if (rc) return rc; }
    HIPC(d.imarks.ensure((size_t)std::max(1, ctx->triCount)));
    HIPC(hipMemsetAsync(d.imarks.p, 0, (size_t)std::max(1, ctx->triCount), st));
    if (d.ichunkCount) hipLaunchKernelGGL(k_mark_triangles, dim3(d.ichunkCount), dim3(256), 0, st, (const float4*)vb_ptr(ctx, VB_NODES, ctx->vcur[VB_NODES]), (const float4*)vb_ptr(ctx, VB_TRIVERTS, ctx->vcur[VB_TRIVERTS]),
                                           ctx->descs.as<GpuBlasDesc>(), (const uint2*)d.ichunks.as<uint2>(), d.imarks.as<uint8_t>());
    HIPC(hipGetLastError());
    d.mark(MARKS);
    return IDKPT_OK;
}

// ---- DScene::pairNodes (k_pair_nodes) for k_trace2's FAST node step: one-BLAS scenes, one scene version; stream-ordered in front of the batch that is about to be launched ----------
static int pair_nodes_prepare(dev_ctx* ctx)
{
    DerivedScene& d = ctx->derived;
    if (d.holds(PAIR)) return IDKPT_OK;
    { int rc = chunks_ensure(ctx); if (rc) return rc; }
    HIPC(d.pairNodes.ensure((size_t)std::max(1, ctx->nodeCount) * 32 + 64));
    if (d.ichunkCount) hipLaunchKernelGGL(k_pair_nodes, dim3(d.ichunkCount), dim3(256), 0, ctx->stream, (const float4*)vb_ptr(ctx, VB_NODES, ctx->vcur[VB_NODES]), ctx->descs.as<GpuBlasDesc>(),
                                           (const uint2*)d.ichunks.as<uint2>(), d.pairNodes.as<float4>());
    HIPC(hipGetLastError());
    d.mark(PAIR);
    return IDKPT_OK;
}

// ---- the packet walk (kernels_packet.hpp): the counters' mirror and the marks its leaf phase reads (who decides: host_launch.hpp packet_decide) ----------------------------------
static int packet_prepare(dev_ctx* ctx)
{
    { int rc = totals_ensure(ctx); if (rc) return rc; }
    HIPC(ctx->derived.pkStats.ensure());
    return marks_prepare(ctx);
}

// ---- the library's own TLAS for the instance loop, and the unified tree (kernels_trace_inst.hpp; k_braid / k_unify_* in kernels_scene.hpp); who wants them: walk_plan.hpp ----------
// The unified tree additionally needs every BLAS used by at most one instance (a scene-wide triangle index then names its instance) and every instance under the same InvModel —
// both decided on the host (instances and transforms only ever arrive through it).
static int inst_unify_prepare(dev_ctx* ctx, const walk::WalkInputs& in)
{
    DerivedScene& d = ctx->derived;
    d.rederiving(OWN_TLAS); d.uniMode = 0;
    if (!walk::inst_unify_wanted(in)) return IDKPT_OK;
    const int n = ctx->instanceCount, nb = (int)ctx->hDescs.size();
    hipStream_t st = ctx->stream;
    if (!d.holds(UNI_TABS)) {                           // once per upload: each BLAS used at most once?  The per-BLAS tables in ascending order of TriangleOffset
        std::vector<int> user(nb, -1);
        bool ok = (int)ctx->hInstances.size() == n;
        for (int i = 0; i < n && ok; i++) { const int b = (int)ctx->hInstances[i].BlasId; if (b < 0 || b >= nb || user[b] >= 0) ok = false; else user[b] = i; }
        d.uniEligible = ok; d.mark(UNI_TABS);
        if (ok) {
            std::vector<int> order(nb); for (int b = 0; b < nb; b++) order[b] = b;
            std::sort(order.begin(), order.end(), [&](int a, int b) { return ctx->hDescs[a].TriangleOffset < ctx->hDescs[b].TriangleOffset; });
            std::vector<uint32_t> tab(2 * (size_t)nb);
            for (int k = 0; k < nb; k++) { tab[k] = (uint32_t)ctx->hDescs[order[k]].TriangleOffset; tab[nb + k] = user[order[k]] >= 0 ? (uint32_t)ctx->hInstances[user[order[k]]].MeshTransformId : 0u; }
            HIPC(d.uTabs.ensure(tab.size() * 4 + 16));
            HIPC(hipMemcpyAsync(d.uTabs.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st)); HIPC(hipStreamSynchronize(st));   // (tab is a stack vector)
        }
    }
    bool same = d.uniEligible && (int)ctx->hInstances.size() == n;
    if (same) {   // every instance's InvModel (rows 3-5 of its GpuMeshTransform) is instance 0's, bit for bit?  On the host's copy: transforms only ever arrive through the host
        const size_t xb = sizeof(GpuMeshTransform);
        const size_t t0 = (size_t)ctx->hInstances[0].MeshTransformId;
        if ((t0 + 1) * xb > ctx->hXforms.size()) same = false;
        for (int i = 1; i < n && same; i++) {
            const size_t ti = (size_t)ctx->hInstances[i].MeshTransformId;
            if ((ti + 1) * xb > ctx->hXforms.size() || memcmp(ctx->hXforms.data() + ti * xb + 48, ctx->hXforms.data() + t0 * xb + 48, 48) != 0) same = false;
        }
    }
    // one space: the unified tree (TREE 1).  Otherwise — different transforms, or a BLAS instanced several times — the general array (TREE 2, option inst_general): a world-space top
    // whose entries take the ray into their instance's space
    const int mode = walk::unify_mode(same, n, ctx->opt.instGeneral);
    if (mode == 0) return IDKPT_OK;
    HIPC(d.uni.ensure());
    { int rc = chunks_ensure(ctx); if (rc) return rc; }
    const float4* nodes = (const float4*)vb_ptr(ctx, VB_NODES, ctx->vcur[VB_NODES]);
    const float4* xf = (const float4*)vb_ptr(ctx, VB_XFORMS, ctx->vcur[VB_XFORMS]);
    const int cap = std::max(n, std::min(ctx->opt.instUnify, 16384)), nodeCount = 2 * cap - 1;
    // the array: [0, 2 cap) the top; TREE 2: [2 cap, 4 cap) one stub pair per entry, then the RESTORE pair; then every BLAS's nodes
    const uint32_t stubBase = 2u * (uint32_t)cap, restoreIdx = 4u * (uint32_t)cap, baseB = mode == 2 ? 4u * (uint32_t)cap + 2u : 2u * (uint32_t)cap;
    // k_braid's entries, areas, leaf boxes, count; k_tlas_build's scratch; the PLOC top; the unified nodes
    const size_t entOff = 0, areaOff = entOff + (size_t)cap * 8, bleafOff = (areaOff + (size_t)cap * 4 + 15) & ~(size_t)15, cntOff = bleafOff + (size_t)cap * 32;
    const size_t ubOff = cntOff + 16;
    const size_t scOff = (ubOff + (size_t)cap * 4 + 255) & ~(size_t)255, leafOff = (size_t)nodeCount * 32, keyOff = leafOff + (size_t)cap * 32, prefOff = keyOff + (size_t)cap * 4;
    HIPC(d.uniBuf.ensure(scOff + prefOff + (size_t)nodeCount * 4)); HIPC(d.utlas.ensure((size_t)nodeCount * 32));      // (its own buffers: the caller's launches on tlasScratch / braidBuf are in flight)
    HIPC(d.unodes.ensure(((size_t)baseB + (size_t)ctx->nodeCount) * 32 + 64));
    if (mode == 2) HIPC(d.uniEntRec.ensure((size_t)cap * 96));
    char* bb = d.uniBuf.as<char>(); char* sc = bb + scOff;
    hipLaunchKernelGGL(k_braid, dim3(1), dim3(TLAS_BUILD_THREADS), 0, st, nodes, ctx->descs.as<GpuBlasDesc>(), ctx->instances.as<GpuBlasInstance>(), xf, n, cap,
                       (uint2*)(bb + entOff), (float*)(bb + areaOff), mode == 2 ? d.uniEntRec.as<float4>() : (float4*)nullptr, (float4*)(bb + bleafOff), (int*)(bb + cntOff), mode == 1 ? 1 : 0, (int*)(bb + ubOff));
    BraidOut bo{(const float4*)(bb + bleafOff), (const int*)(bb + cntOff), (const int*)(bb + ubOff)};
    hipLaunchKernelGGL(k_tlas_build, dim3(1), dim3(TLAS_BUILD_THREADS), 0, st, nodes, ctx->descs.as<GpuBlasDesc>(), ctx->instances.as<GpuBlasInstance>(), xf, n, ctx->opt.instUnifyRadius,
                       d.utlas.as<float4>(), (float4*)sc, (float4*)(sc + leafOff), (uint32_t*)(sc + keyOff), (int*)(sc + prefOff), 1, d.uni.dev_as<float>(), 0, bo);
    hipLaunchKernelGGL(k_unify_top, dim3(1), dim3(TLAS_BUILD_THREADS), 0, st, (const float4*)d.utlas.as<float4>(), (const int*)(bb + cntOff), (const uint2*)(bb + entOff), nodes, ctx->descs.as<GpuBlasDesc>(),
                       ctx->instances.as<GpuBlasInstance>(), baseB, d.unodes.as<float4>(), mode == 2 ? 1 : 0, stubBase, restoreIdx);
    if (d.ichunkCount) hipLaunchKernelGGL(k_unify_blas, dim3(d.ichunkCount), dim3(256), 0, st, nodes, ctx->descs.as<GpuBlasDesc>(), (const uint2*)d.ichunks.as<uint2>(), baseB, d.unodes.as<float4>());
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(st));                       // (waited for: the entries and the top's depth size this walk's stack; a re-derivation — transforms, refits — is rare on the scenes that use it)
    const volatile float* h = d.uni.host_as<float>();
    d.uniEntries = (int)h[1]; d.uniDepth = (int)h[2];
    d.mark(UNI, d.uniDepth > 0 && d.uniEntries >= n);
    d.uniMode = d.holds(UNI) ? mode : 0; d.uniBaseB = baseB; d.uniRestoreIdx = restoreIdx;
    // rows of this walk's stack: what the device derived from the BLASes' RequiredStackSize (validated >= the trees' real need at upload) and the top above them, never more than
    // "the deepest BLAS under the whole top" (a ray that needs more rows is flagged and traced by the exact loop).  TREE 2: an entry parks the node the lane was about to visit and the
    // RESTORE pair under its subtree
    const int extra = mode == 2 ? 3 : 1;
    const int loose = std::max(1, ctx->st.BlasStackSize > 0 ? ctx->st.BlasStackSize : ctx->sceneStack) + std::max(1, d.uniDepth) + extra;
    d.uniCap = std::min(96, std::max(4, std::min(loose, h[3] > 0.0f ? (int)h[3] + extra : loose)));
    return IDKPT_OK;
}

// derives what is stale of what walk::inst_walk looks at to decide how a several-instance scene without UseTlas is traced: the own TLAS, the unified tree, whether the tree / the sieve
// is worth it (TLAS_BUILT, isieveWorth).  The instances' overlap is measured on the device into host-mapped memory; the first measurement after an upload is
// waited for, later ones (animated transforms) are read whenever they have arrived — the decision only moves time, never a result
static int inst_tlas_derive(dev_ctx* ctx, const walk::WalkInputs& in)
{
    DerivedScene& d = ctx->derived;
    const bool wantOwn = walk::inst_tlas_wanted(in), wantU = walk::inst_unify_wanted(in);
    const bool wantT = wantOwn || wantU, wantS = walk::inst_tlas_wanted(in, true);     // (the unified tree's launches use the own TLAS's top boxes for the primary rays' pre-cull, k_gen_primary)
    if (!wantT && !wantS) return IDKPT_OK;
    { int rc = totals_ensure(ctx); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    const float4* nodes = (const float4*)vb_ptr(ctx, VB_NODES, ctx->vcur[VB_NODES]);
    const int n = ctx->instanceCount;
    HIPC(d.overlap.ensure());
    if (!d.holds(OWN_TLAS)) {
        // partial re-braiding (k_braid): the tree's leaves are subtrees of the instances' BLASes, at most `cap` of them
        const bool braid = wantT && ctx->opt.instBraid > 0 && ctx->sceneNested;
        const int cap = braid ? std::max(n, std::min(ctx->opt.instBraid, 8192)) : n, nodeCount = 2 * cap - 1;
        const size_t leafOff = (size_t)nodeCount * 32, keyOff = leafOff + (size_t)cap * 32, prefOff = keyOff + (size_t)cap * 4;
        HIPC(ctx->tlasScratch.ensure(prefOff + (size_t)nodeCount * 4)); HIPC(d.itlas.ensure((size_t)nodeCount * 32));
        char* sc = ctx->tlasScratch.as<char>();
        const float4* xf = (const float4*)vb_ptr(ctx, VB_XFORMS, ctx->vcur[VB_XFORMS]);
        BraidOut bo{nullptr, nullptr};
        if (braid) {
            const size_t entOff = 0, areaOff = entOff + (size_t)cap * 8, bleafOff = (areaOff + (size_t)cap * 4 + 15) & ~(size_t)15, cntOff = bleafOff + (size_t)cap * 32;
            HIPC(d.braidBuf.ensure(cntOff + 16)); HIPC(d.entRec.ensure((size_t)cap * 96));
            char* bb = d.braidBuf.as<char>();
            hipLaunchKernelGGL(k_braid, dim3(1), dim3(TLAS_BUILD_THREADS), 0, st, nodes, ctx->descs.as<GpuBlasDesc>(), ctx->instances.as<GpuBlasInstance>(), xf, n, cap,
                               (uint2*)(bb + entOff), (float*)(bb + areaOff), d.entRec.as<float4>(), (float4*)(bb + bleafOff), (int*)(bb + cntOff));
            HIPC(hipGetLastError());
            bo.leaf = (const float4*)(bb + bleafOff); bo.count = (const int*)(bb + cntOff);
        }
        const volatile float* h = d.overlap.host_as<float>();                // [0] the leaves' boxes a random line meets, [1] the leaves, [2] the built tree's depth
        auto itlas_build = [&](int leavesOnly) { launch(k_tlas_build, dim3(1), dim3(TLAS_BUILD_THREADS), 0, st, nodes, ctx->descs.as<GpuBlasDesc>(), ctx->instances.as<GpuBlasInstance>(), xf, n, 15 /* TLAS.cs: SearchRadius */,
                                                        d.itlas.as<float4>(), (float4*)sc, (float4*)(sc + leafOff), (uint32_t*)(sc + keyOff), (int*)(sc + prefOff), 1, d.overlap.dev_as<float>(), leavesOnly, bo); };
        itlas_build(1);                                                       // the overlap of the boxes as they are now
        HIPC(hipGetLastError());
        const bool first = !d.holds(OVERLAP_KNOWN);
        if (first) { HIPC(hipStreamSynchronize(st)); d.mark(OVERLAP_KNOWN); }
        { int rc = inst_unify_prepare(ctx, in); if (rc) return rc; }
        const float met = h[0] * 100.0f;                                     // percent of the leaves' boxes a random line meets, x their number
        const float leavesRead = h[1], leaves = braid ? std::max((float)n, leavesRead) : (float)n;
        const bool worth = d.holds(UNI) || (wantOwn && (ctx->opt.instTlasOverlap >= 100 || met <= (float)ctx->opt.instTlasOverlap * leaves));
        if (worth) { itlas_build(0); HIPC(hipGetLastError()); if (first) HIPC(hipStreamSynchronize(st)); }   // (the first build's depth is waited for; later ones are read when they have arrived)
        d.mark(TLAS_BUILT, worth); d.itlasBraided = worth && braid; d.itlasEntries = (int)leaves;
        d.itlasDepth = worth ? (int)h[2] : 0;
        float metInst = met;                                                 // the sieve's question is about whole instances
        if (braid && !worth && wantS) { bo = BraidOut{nullptr, nullptr}; itlas_build(1); HIPC(hipGetLastError()); if (first) HIPC(hipStreamSynchronize(st)); metInst = h[0] * 100.0f; }
        d.isieveWorth = !worth && wantS && (ctx->opt.instSieveOverlap >= 100 || metInst <= (float)ctx->opt.instSieveOverlap * (float)n);
        d.itlasNeed = inst_tlas_rows(ctx);                                   // (a ray that needs more rows is traced by the exact loop)
        d.mark(OWN_TLAS);                                                    // (the options that change what is wanted invalidate the decision: host_options.hpp)
    }
    return IDKPT_OK;
}
