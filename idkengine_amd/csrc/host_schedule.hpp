// host_schedule.hpp — PathTracer.Compute: the launch schedule of a batch of samples (flush_batch), its deferred last bounce, idkptRender and the batching knobs.
// Part of the single translation unit idkpt.hip (included there, in this order).
#pragma once

// slots: which state of every versioned buffer the kernels read (null: the current one); multi: the batch's samples saw different states -> the pointers are the
// arena bases and DScene::ver holds every sample's offsets (VER kernels)
static DScene make_dscene(dev_ctx* ctx, const uint8_t* slots, bool multi)
{
    DScene s;
    auto at = [&](int b) -> char* { return multi ? (char*)vb_buf(ctx, b).p : vb_ptr(ctx, b, slots ? slots[b] : ctx->vcur[b]); };
    s.nodes = (const float4*)at(VB_NODES); s.tris = ctx->tris.as<uint4>(); s.triVerts = (const float4*)at(VB_TRIVERTS);
    s.descs = ctx->descs.as<GpuBlasDesc>(); s.instances = ctx->instances.as<GpuBlasInstance>(); s.instanceCount = ctx->instanceCount;
    s.tlas = (const float4*)at(VB_TLAS); s.tlasCount = ctx->tlasCount; s.vertices = (const uint4*)at(VB_VERTICES);
    s.instRec = nullptr;        // (set for the batches that walk the library's own TLAS or sieve the instances: trace_plan)
    s.pairNodes = nullptr;      // (set for the batches whose one-BLAS launches take k_trace2's FAST node step: trace_plan)
    s.meshes = ctx->meshes.as<GpuMesh>(); s.materials = ctx->materials.as<GpuMaterial>(); s.xforms = (const float4*)at(VB_XFORMS);
    s.lights = ctx->lights.as<GpuLight>(); s.lightCount = ctx->lightCount; s.sky = ctx->sky.as<float4>(); s.skySize = ctx->skySize;
    s.textures = ctx->texDescs.as<TexDesc>(); s.textureCount = ctx->textureCount; s.srgbLut = ctx->srgbLut.as<float>();
    s.overflow = ctx->dOverflow;
    s.ver = multi ? ctx->verTab.as<uint32_t>() : nullptr;
    return s;
}
static DScene make_dscene(dev_ctx* ctx) { return make_dscene(ctx, nullptr, false); }
static DScene make_dscene_last(dev_ctx* ctx) { return make_dscene(ctx, ctx->lastSlots, ctx->lastMulti); }   // what the last launched batch read (finish_deferred, regeneration of culled rays)

static float4* image_ptr(dev_ctx* ctx, int i, int slot) { return ctx->img[i].as<float4>() + (size_t)slot * ((size_t)ctx->W * ctx->rows); }

// Grid of a traversal launch whose ray count is only known on the device: `prev` = the count the same launch had in the previous batch (host-mapped mirror,
// possibly one batch stale; 0 = unknown -> full grid).  Any grid >= 1 is correct (the waves are persistent); the size only costs or saves time:
//   * never more than hintMul x the waves that hold all rays at once (tiny frames would otherwise spend their time dispatching idle workgroups), at least 256;
//   * launches below ~1.5 rays per lane of the full grid run faster on FEWER, fuller waves — every wave instruction costs the same whatever its exec mask, and a
//     launch this small lasts as long as its longest rays, whose steps get faster when fewer waves share a SIMD: raysX4 / 4 rays per lane, but not below
//     1024 waves where the first rule allows them (round 3, same box: headline one frame at a time +6 %, Cornell 1080p RayDepth 5 +12 %; profiles/r03_trace_experiments.md 7).
//   * launches of up to GRID_MID_RAYS rays (the headline frame with up to ~24 samples in flight, one rank's share of an N-GPU frame) run 2-4 % faster on 20 than on 24
//     waves per CU for the same reason, and views whose launches are that small only with a few samples in flight (every pixel traversing) lose nothing measurable;
//     above it 24 is never worse (profiles/r03_trace_experiments.md 9).
#define GRID_MID_RAYS 14000000u
// Which traversal kernel a launch gets: k_trace2s (kernels_trace_split.hpp: long rays split across the idle lanes of their wave once the work list is empty) pays
// where a launch ends with a few long rays on an otherwise idle chip — launches of up to SPLIT_MAX_RAYS rays (a frame traced alone, the bounce launches of small
// batches, one rank's share of an N-GPU frame); its extra registers (one wave per SIMD less) cost large launches more than their tails are worth.
// Measured (profiles/r04_small_launch_experiments.md): headline view one frame at a time (0.36 M + 0.28 M rays per launch) +8 %, three samples in flight +4 %, one
// rank's share of an 8 / 4-GPU frame +12 % / +5 %; the atrium and the interior view one frame at a time (1.9-2.1 M rays per launch, every pixel traverses) -10 % / -1.5 %.
// So: launches of fewer than SPLIT_MAX_RAYS rays, and only on views where most pixels miss the scene's root box (fewer than half of the primary rays entered the
// traversal in the previous batch) — there the launch time is the dependent chain of the rays that cross the whole scene without hitting anything.
#define SPLIT_MAX_RAYS 1500000u
static bool want_split(const dev_ctx* ctx, uint32_t prev, bool known, int samples)
{
    if (ctx->opt.split == 0) return false;
    if (ctx->opt.split >= 2) return true;
    return known && sparse_view(ctx, samples) && prev > 0u && prev < SPLIT_MAX_RAYS;
}
// k_trace_fused: where a batch's two traversal launches are bound by their longest rays, not by their ray count (the same regime as the split)
// (measured: it saves launches, not chain length — +5 % where one sparse frame is traced alone, a loss everywhere else: kernels_trace_fused.hpp)
#define FUSED_MAX_RAYS 600000u
static bool want_fused(const dev_ctx* ctx, uint32_t prev, bool known, int samples)
{
    if (ctx->opt.fused == 0) return false;
    if (ctx->opt.fused >= 2) return true;
    return known && prev > 0u && prev < FUSED_MAX_RAYS && few_traversed(ctx, prev, std::max(1, samples));
}
// The deferred last bounce traced hit-or-miss (k_trace2 OCCL, kernels_trace.hpp; the argument: DESIGN.md §4) — THE rule, whole: launch_trace2 obeys what this says.
// readsOnlyHitOrMiss: the bounce is deferred and a hit of it cannot add radiance (no emission, no light hits), so k_shade_last<false> reads `T == PT_FLOAT_MAX` of its hit records and
// nothing else (rays whose throughput is not finite aside: write_trace_ready marks them, and the walk keeps a marked lane closest-hit).  Only the plain one-BLAS walk has the flavour:
// Plain or Fast, not the fused launch, not a split one (split: what want_split said of this launch), one scene version, the stock kernels; the counting build keeps the closest-hit
// walk, so its visit counts stay the reference's.  (Frames never run in query mode: idkptTraceRays has its own launch, host_queries.hpp.)
static bool want_occlusion(const dev_ctx* ctx, const TracePlan& plan, bool readsOnlyHitOrMiss, bool split)
{
    return readsOnlyHitOrMiss && ctx->opt.lastOcclusion != 0 && !plan.fused && (plan.walk == Walk::Plain || plan.walk == Walk::Fast) && !(split && plan.splitOk)
           && !plan.multiVer && !plan.counting && !ctx->counters && (ctx->opt.traceVariant == 0 || ctx->opt.traceVariant == 100);
}
// The folded last bounce (option fold_last) — the rule, whole: behind a hit-or-miss launch (tookOccl: want_occlusion above said yes) the only thing anybody reads of the bounce
// before its continuation is asked for is "missed", and k_final_draw is the one reader of the sum that bit decides.  So the launch stores the bit per ray id (PRIMARY instantiation, over the
// pixel-major list or the alive queue: trace_bounce) and no hit records, k_final_draw adds the sky of the misses, and k_shade_last<false> keeps the rays whose throughput is not finite.
// Everything want_occlusion excludes keeps the k_shade_last pass.  (Measured on the default, interior and atrium views: profiles/last_fold.md — no view condition.)
static bool want_fold(const dev_ctx* ctx, bool tookOccl) { return tookOccl && ctx->opt.foldLast != 0; }
// ... and what the kernels that produce the rays of a last bounce are told before its launch is decided (Frame::markLast): whether it can still come out folded
static bool may_fold(const dev_ctx* ctx, bool deferLast, bool deferAllHits) { return deferLast && !deferAllHits && ctx->opt.lastOcclusion != 0 && ctx->opt.foldLast != 0; }
static uint32_t small_launch_grid(uint32_t fullGrid, uint32_t prev, int hintMul, int raysX4, uint32_t midGrid)
{
    if (prev == 0u || hintMul <= 0) return fullGrid;
    const uint32_t cap = std::max<uint32_t>(256u, (uint32_t)(((uint64_t)hintMul * prev + 63) / 64));
    uint32_t g = cap;
    if (raysX4 > 0) g = std::max<uint32_t>((uint32_t)(((uint64_t)prev * 4u / (uint32_t)raysX4 + 63) / 64), std::min<uint32_t>(cap, 1024u));
    if (midGrid > 0u && prev < GRID_MID_RAYS) g = std::min(g, midGrid);
    return std::min(fullGrid, std::min(g, cap));
}

// What a batch carries from stage to stage of flush_batch (and what finish_deferred rebuilds of it for the batch before).
struct Batch {
    dev_ctx* ctx; hipStream_t st; int B, depth; uint32_t N, Npad, total, gridTotal, scanBlocks;        // samples, RayDepth, pixels per sample, their padded pitch, B x Npad, its 256-thread blocks, its scan blocks
    bool multiVer, fast, debug, capturing;
    Frame f; DScene s; TracePlan plan;
    RayBufs rays; HitBufs hits; TraceBufs tr, trNone;
    uint32_t* counts; uint32_t* bases /* [MAX_DEPTH_SLOTS][MAX_BATCH + 1] */; uint32_t* work; uint64_t* counters; uint32_t* hostCounts; uint32_t* hostBases;   // (host*: the host-mapped mirrors)
    unsigned long long* contMask; uint32_t* waveLocal /* per-wave exclusive offset inside its 256-wave scan block */; uint32_t* blockSums; uint32_t* keysTmp;
    uint32_t* activeList; uint32_t* activeCount;                         // FirstHit's work list: scratch (capacity uints), free until the first sort
    uint32_t* pmList; uint32_t* pmCount; bool pmBounce;                  // (RayDepth < MAX_DEPTH_SLOTS - 2, idkptSetSettings: the word is nobody's queue length — k_scan_blocks writes counts[1 .. RayDepth]; reset with the others)
    const uint8_t* tileClass; uint32_t midGrid, traceGrid;              // per-tile pre-classification of this batch (fast path with pre-cull only); the grids of its traversal launches
    int side;                                                            // queue[side] holds the rays entering bounce j, its length is counts[j], sample k starts at bases[j][k]
};
static const int BS = MAX_BATCH + 1;                                     // pitch of bases[]

// the views of the wavefront buffers and the sizes that follow from B samples of pitch Npad
static void batch_views(dev_ctx* ctx, Batch& b, int B, uint32_t Npad)
{
    b.ctx = ctx; b.st = ctx->stream; b.B = B; b.depth = ctx->st.RayDepth; b.N = (uint32_t)((size_t)ctx->W * ctx->rows); b.Npad = Npad; b.total = (uint32_t)B * Npad;
    b.gridTotal = (b.total + 255) / 256; b.scanBlocks = ((b.total + 63) / 64 + SCAN_WAVES_PER_BLOCK - 1) / SCAN_WAVES_PER_BLOCK;
    b.rays = {ctx->rayO.as<float4>(), ctx->rayT.as<float4>(), ctx->rayR.as<float4>(), ctx->aovA.as<float4>(), ctx->aovN.as<float4>(), ctx->contFlag.as<uint8_t>()}; b.hits = {ctx->hit.as<float4>(), ctx->hitCost.as<float>()};
    b.tr = {ctx->trRec.as<float4>(), nullptr, nullptr, ctx->deferCount.as<uint32_t>() + 1}; b.trNone = {nullptr, nullptr, nullptr, nullptr};
    b.counts = ctx->counts.as<uint32_t>(); b.bases = ctx->bases.as<uint32_t>(); b.work = ctx->work.as<uint32_t>(); b.counters = ctx->counters64.as<uint64_t>(); b.hostCounts = ctx->dCountsMirror; b.hostBases = ctx->dBasesMirror;
    b.contMask = ctx->contMask.as<unsigned long long>(); b.waveLocal = ctx->waveCounts.as<uint32_t>(); b.blockSums = ctx->blockSums.as<uint32_t>(); b.keysTmp = ctx->keysTmp.as<uint32_t>();
    b.activeList = ctx->sortVals.as<uint32_t>(); b.activeCount = b.counts + (MAX_DEPTH_SLOTS - 1);
    b.pmList = nullptr; b.pmCount = b.counts + (MAX_DEPTH_SLOTS - 2); b.pmBounce = false; b.tileClass = nullptr; b.side = 1; b.capturing = false;
}

// The tail of bounce j: shading, scan and scatter of queue q (*cnt entries) into the other side's queue; counts[j + 1], bases[j + 1] and their mirrors are written.
// gbase: the multi-GPU sample bases (null: single context); traced: the traced-rays counter (null: not counted); record: evBounce[j + 1] is recorded once bases[j + 1] is final.
static int bounce_tail(Batch& b, int j, const uint32_t* q, const uint32_t* cnt, const uint32_t* gbase, unsigned long long* traced, bool record, const TraceBufs& tr)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st; const int side = b.side;
    with_flag(b.multiVer, [&](auto VER) { launch(k_shade<false, VER>, dim3(b.gridTotal), dim3(256), 0, st, b.s, b.f, b.rays, tr, b.hits, q, cnt, 0u, b.bases + j * BS, gbase, b.contMask, b.waveLocal, b.keysTmp); });
    launch(k_scan_local<false>, dim3(b.scanBlocks), dim3(SCAN_WAVES_PER_BLOCK), 0, st, cnt, 0u, nullptr, b.contMask, b.waveLocal, b.blockSums);
    launch(k_scan_blocks, dim3(1), dim3(1024), 0, st, cnt, 0u, b.blockSums, b.waveLocal, b.counts + j + 1, traced, b.contMask, b.bases + j * BS, b.Npad, b.B, b.bases + (j + 1) * BS, b.hostCounts + j + 1, b.hostBases + (size_t)(j + 1) * BS, nullptr, nullptr);
    if (record) HIPC(hipEventRecord(ctx->evBounce[j + 1], st));
    launch(k_compact<false>, dim3(b.gridTotal), dim3(256), 0, st, q, cnt, 0u, b.contMask, b.waveLocal, b.blockSums, b.keysTmp, ctx->queue[1 - side].as<uint32_t>(), ctx->keys[1 - side].as<uint32_t>());
    return IDKPT_OK;
}

// The continuation of a deferred last bounce (k_shade_last): the radiance k_shade_last replaced goes back, then the bounce's tail runs — shading, scan, scatter —
// on the inputs the batch left untouched (hit records, ray state, the queue entering the bounce, its per-sample bases).  Afterwards ray state, alive
// queue and counts are what the eager path leaves, bit for bit; the frame was complete before.
static int finish_deferred(dev_ctx* ctx)
{
    if (!ctx->defer.valid) return IDKPT_OK;
    ctx->defer.valid = false;
    Batch b; batch_views(ctx, b, ctx->defer.B, ctx->defer.Npad);
    b.side = ctx->defer.side; b.f = ctx->lastFrame; b.f.markLast = 0; b.f.foldLast = 0; b.s = make_dscene_last(ctx); b.multiVer = ctx->lastMulti;           // the scene states the deferred batch was traced with (its slots are pinned until now: ver_writable)
    const uint32_t* q = ctx->queue[b.side].as<uint32_t>(); const uint32_t* cnt = ctx->deferCount.as<uint32_t>();               // (counts[j] itself was reset by the batch's last kernel)
    if (ctx->defer.occl) {
        // the bounce was traced hit-or-miss (k_trace2 OCCL): its closest hits first — the plain closest-hit kernel over the same list, the same records (trRec and the pixel-major list belong
        // to batches alone, and the next batch drops this continuation before it touches them), the same hit indexing.  Nothing of it is counted: RaysTraced counted the bounce at its scan,
        // TraceLaunches / TraceMsTotal come from events recorded around a batch's launches.  The launch's work-list words are zero (k_final_draw reset them) unless something left them dirty.
        const int j = ctx->defer.j;
        if (ctx->countersDirty) HIPC(hipMemsetAsync(b.work, 0, WORK_WORDS * 4, b.st));
        // The plan is Plain on purpose, whatever the batch walked: Plain reads s.nodes only — pinned for the deferred batch — and so does not depend on DScene::pairNodes still being
        // derived, and its hits are FAST's bit for bit (kernels_trace.hpp).  Every other field of the plan is off: no packets, nothing fused, one version, no counting, no split.
        TracePlan p{}; p.walk = Walk::Plain; p.ldsBytes = ctx->defer.ldsBytes; p.grid = ctx->defer.grid;
        Frame ft = b.f; if (ctx->defer.pm) ft.hitsByRid = 0;                  // (the PRIMARY instantiations read a list of ray ids and store per ray id: trace_bounce)
        if (ctx->defer.pm) launch_trace2<true>(ctx, p, p.grid, b.st, b.s, ft, b.rays, b.tr, b.hits, ctx->defer.list, cnt, b.work + j, b.counters, false, j);
        else launch_trace2<false>(ctx, p, p.grid, b.st, b.s, ft, b.rays, b.tr, b.hits, q, cnt, b.work + j, b.counters, false, j);
        ctx->defer.occl = false;
    }
    with_flag(ctx->defer.allHits, [&](auto ALL) { launch(k_restore_last<ALL>, dim3(b.gridTotal), dim3(256), 0, b.st, b.rays, b.hits, q, cnt, ctx->radSave.as<float4>(), b.f.hitsByRid, ctx->defer.fold ? 1 : 0); });
    { int rc = bounce_tail(b, ctx->defer.j, q, cnt, nullptr, nullptr, false, b.tr); if (rc) return rc; }
    HIPC(hipGetLastError());
    ctx->lastQueueSide = 1 - b.side; ctx->countersDirty = true;                                          // (counts[j + 1] was written after the batch's reset: the next batch clears its counters itself)
    return IDKPT_OK;
}

// ---- the stages of flush_batch, in the order of PathTracer.Compute ------------------------------------------------------------------------------------------------------
// Which state of the geometry every sample sees (scene versions): one for all -> plain pointers; else a per-sample table of offsets into the arenas (VER kernels).
// Frame ring: every sample renders with the camera it was queued with.  Both tables go through pinned double-buffered staging (PinnedStage).
static int stage_versions_cameras(Batch& b)
{
    dev_ctx* ctx = b.ctx; const int B = b.B;
    bool multiVer = false; for (int k = 1; k < B && !multiVer; k++) multiVer = memcmp(ctx->pending[k].vs, ctx->pending[0].vs, VB_COUNT) != 0;
    for (int v = 0; v < VB_COUNT; v++) { uint64_t m = 0; for (int k = 0; k < B; k++) m |= 1ull << ctx->pending[k].vs[v]; ctx->lastMask[v] = m; ctx->lastSlots[v] = ctx->pending[0].vs[v]; }
    ctx->lastMulti = b.multiVer = multiVer;
    auto fillVersions = [&](char* half) {
        for (int k = 0; k < B; k++) {
            const uint8_t* vs = ctx->pending[k].vs; uint32_t* row = (uint32_t*)half + (size_t)k * SCENE_VER_WORDS;
            for (int v = 0; v < VB_COUNT; v++) row[v] = (uint32_t)(((size_t)vs[v] * ctx->vstride[v]) / 16);   // 16-byte units
            for (int v = VB_COUNT; v < SCENE_VER_WORDS; v++) row[v] = 0u;
        } };
    if (multiVer) HIPC(ctx->verStage.stage(ctx->verTab, (size_t)MAX_BATCH * SCENE_VER_WORDS * 4, (size_t)B * SCENE_VER_WORDS * 4, b.st, fillVersions));
    b.s = make_dscene_last(ctx);
    memset(&b.f, 0, sizeof(b.f));                                        // (every field a kernel variant may look at has a defined value: queryMode, hitsByRid, ...)
    if (ctx->ringSize > 1) {
        auto fillCameras = [&](char* half) { for (int k = 0; k < B; k++) memcpy(half + (size_t)k * 36 * 4, ctx->pending[k].cam, 36 * 4); };
        HIPC(ctx->camStage.stage(ctx->camTab, (size_t)MAX_BATCH * 36 * 4, (size_t)B * 36 * 4, b.st, fillCameras));
        b.f.cams = ctx->camTab.as<float>();
    }
    return IDKPT_OK;
}

#ifdef IDKPT_DEVELOPER
// "graph_probe" (developer build): is a hipGraph of a batch's launches faster than the launches?  The batch is captured instead of executed, then
// executed once as a graph and replayed graph_probe times between two events (the replays re-accumulate the same sample: timing only).
static void graph_probe_begin(Batch& b) { if (b.ctx->opt.graphProbe > 0 && !b.ctx->timing) b.capturing = hipStreamBeginCapture(b.st, hipStreamCaptureModeThreadLocal) == hipSuccess; }
static void graph_probe_end(Batch& b)
{
    if (!b.capturing) return;
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st;
    hipGraph_t g = nullptr; hipGraphExec_t ex = nullptr; const int K = ctx->opt.graphProbe; ctx->opt.graphProbe = 0;
    if (hipStreamEndCapture(st, &g) == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess) {
        hipEvent_t e0 = nullptr, e1 = nullptr; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        (void)hipGraphLaunch(ex, st); (void)hipStreamSynchronize(st);                       // the batch itself (a capture does not execute)
        (void)hipEventRecord(e0, st);
        for (int k = 0; k < K; k++) (void)hipGraphLaunch(ex, st);
        (void)hipEventRecord(e1, st); (void)hipStreamSynchronize(st);
        float ms = 0.0f; (void)hipEventElapsedTime(&ms, e0, e1);
        size_t nodes = 0; (void)hipGraphGetNodes(g, nullptr, &nodes);
        fprintf(stderr, "[idkpt graph] batch of %d sample(s) captured: %zu graph nodes; %d replays: %.1f us per batch\n", b.B, nodes, K, ms * 1000.0f / (float)K);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipGraphExecDestroy(ex);
    } else fprintf(stderr, "[idkpt graph] capture or instantiation failed: %s\n", hipGetErrorString(hipGetLastError()));
    if (g) (void)hipGraphDestroy(g);
}
#else
static void graph_probe_begin(Batch&) {}
static void graph_probe_end(Batch&) {}
#endif

// The Frame the kernels of this batch see, the reset of the batch counters, how the batch is traced (trace_plan) and the grids of its launches.
static int frame_setup(Batch& b)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st; Frame& f = b.f; const int B = b.B;
    memcpy(f.invProj, ctx->pending[0].cam, 64); memcpy(f.invView, ctx->pending[0].cam + 16, 64); memcpy(f.viewPos, ctx->pending[0].cam + 32, 12);   // the camera the samples were queued with
    f.W = ctx->W; f.H = ctx->H; f.rowMod = ctx->rowMod; f.rowRem = ctx->rowRem; f.rows = ctx->rows; f.rowBandLog2 = ctx->rowBandLog2;
    f.g = ctx->st.Gpu; f.useTlas = ctx->st.UseTlas; f.stackCap = std::max(1, ctx->st.BlasStackSize > 0 ? ctx->st.BlasStackSize : ctx->sceneStack);
    f.outputAovs = ctx->st.OutputAOVs; f.batch = B; f.Npad = b.Npad;
    HIPC(ctx->trRec.ensure((size_t)ctx->maxBatch * b.Npad * 64)); b.tr.rec = ctx->trRec.as<float4>();
    for (int k = 0; k < MAX_BATCH; k++) { f.accum[k] = k < B ? ctx->pending[k].accum : 0u; f.slotOf[k] = (uint32_t)(k < B ? ctx->pending[k].slot : 0); }
    f.seqFirst = ctx->seqFirst; f.seqStride = ctx->seqStride; f.accumulated = f.seqFirst + f.accum[0] * f.seqStride;
    f.tilePerSample = (f.cams != nullptr || b.multiVer) ? 1 : 0;
    graph_probe_begin(b);                                          // (developer build; from here on the batch may be captured instead of executed)
    if (ctx->timing) HIPC(hipEventRecord(ctx->evFrame[0], st));
    ctx->defer.valid = false;                                      // (a deferred last bounce of the previous batch that nobody asked for: its buffers are reused now)
    if (ctx->countersDirty) { HIPC(hipMemsetAsync(b.work, 0, WORK_WORDS * 4, st)); HIPC(hipMemsetAsync(b.counts, 0, MAX_DEPTH_SLOTS * 4, st)); HIPC(hipMemsetAsync(b.tr.oddCount, 0, 4, st)); }   // (otherwise the previous batch's k_final_draw has reset them)
    ctx->countersDirty = true;
    f.tlasCap = std::min(TLAS_STACK_SIZE, std::max(1, ctx->tlasNeed));
    f.grabUnitLog2 = std::min(24, std::max(6, ctx->opt.grabUnitLog2)); f.grabFixed = std::max(0, ctx->opt.grabFixed);   // work-list hand-out (kernels_trace.hpp)
    f.leafMin = ctx->opt.leafMin > 0 ? ctx->opt.leafMin : (B >= 4 ? 16 : 12);        // (measured: 16-20 with many samples in flight, 12 for a frame traced alone; tools/sweep_sched.py)
    b.fast = fast_path(ctx);
    // (not where the samples of a batch are different frames — their own cameras or scene versions: the same pixel is then not the same ray, and under scene versions not even the
    // same node addresses; measured on the animated bench, 8 / 32 frames in flight: 3 291 / 3 716 -> 3 011 / 3 117 Mray/s)
    f.genPixelMajor = (b.fast && ctx->opt.genPixelMajor > 0 && B >= ctx->opt.genPixelMajor && !f.tilePerSample) ? 1 : 0;
    // how this batch is traced (host_launch.hpp trace_plan): walk, packets, fusion, LDS bytes and the persistent grid — as many 1-wave workgroups as the chip holds, but never more waves than the launch can have rays (small frames would spend their time dispatching idle workgroups)
    { int rc = trace_plan(ctx, f, b.s, b.multiVer, false, false, b.plan); if (rc) { ctx->pending.clear(); return rc; } }
    b.traceGrid = std::min<uint32_t>(b.plan.grid, std::max<uint32_t>(1u, (uint32_t)(((size_t)B * b.N + 63) / 64)));
    b.midGrid = (ctx->opt.gridMidWaves > 0 && ctx->opt.traceWaves == 0) ? (uint32_t)(ctx->numCUs * std::min(b.plan.wavesPerCU, ctx->opt.gridMidWaves)) : 0u;   // (an explicit trace_waves wins)
    f.gridRaysX4 = (uint32_t)std::max(0, ctx->opt.gridRaysX4); f.gridMid = b.midGrid; f.gridMidRays = GRID_MID_RAYS; f.splitMode = (ctx->opt.split == 3 ? 2 : 1) | (ctx->opt.splitDonor ? 4 : 0); f.poolMin = ctx->opt.poolMin; f.advMin = ctx->opt.advMin > 0 ? ctx->opt.advMin : (B >= 4 ? 8 : 1); f.splitPeek = ctx->opt.splitPeek;   // the same rules inside k_trace2, on the launch's actual ray count
    b.debug = f.g.DoDebugBVHTraversal != 0; f.shadeMin = ctx->opt.fusedShadeMin; f.scatterLog2 = ctx->opt.splitScatter;
    if (!b.fast && (B != 1 || b.multiVer)) { ctx->pending.clear(); return fail(ctx, IDKPT_ERR_UNKNOWN, "internal: generic path is never batched"); }
    return IDKPT_OK;
}

// FirstHit's tail on both paths: the scan over every ray slot and the scatter of the continuing rays into queue[1]
static int first_hit_compact(Batch& b)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st;
    launch(k_scan_blocks, dim3(1), dim3(1024), 0, st, nullptr, b.total, b.blockSums, b.waveLocal, b.counts + 1, (unsigned long long*)(1 < b.depth ? b.counters + 2 : nullptr), b.contMask, nullptr, b.Npad, b.B, b.bases + 1 * BS, b.hostCounts + 1, b.hostBases + 1 * BS, b.counts + MAX_DEPTH_SLOTS - 1, b.hostCounts + MAX_DEPTH_SLOTS - 1);
    if (ctx->evBounce) HIPC(hipEventRecord(ctx->evBounce[1], st));      // bases[1] (alive counts entering bounce 1) are final
    launch(k_compact<true>, dim3(b.gridTotal), dim3(256), 0, st, nullptr, nullptr, b.total, b.contMask, b.waveLocal, b.blockSums, b.keysTmp, ctx->queue[1].as<uint32_t>(), ctx->keys[1].as<uint32_t>());
    return IDKPT_OK;
}

// FirstHit on the fast path: tile classes, primary rays, their traversal (or the fused launch), the first shading
static int first_hit_fast(Batch& b)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st; Frame& f = b.f; const DScene& s = b.s; const int B = b.B; const uint32_t N = b.N;
    const uint32_t tilesX = ((uint32_t)f.W + 7) / 8, tilesY = ((uint32_t)f.rows + 7) / 8; const uint32_t genWaves = tilesX * tilesY;
    const int cull = f.g.DoTraceLights ? 0 : 1;
    // single instance without lights: k_trace2 reads nothing but the trace-ready record, so the planes of a surviving primary ray need not exist before k_shade_first
    const int lean = (cull && !f.useTlas && s.instanceCount == 1 && ctx->opt.noLeanPrimary == 0) ? 1 : 0;
    uint8_t* contFlag = ctx->contFlag.as<uint8_t>();
    if (ctx->capturePrimary) launch(k_fill_miss, dim3((N + 255) / 256), dim3(256), 0, st, b.hits, (size_t)(B - 1) * b.Npad, N);
    if (cull && !ctx->opt.noTileCull) {   // sample-independent pre-classification of the 8x8 tiles (conservative whole-tile miss test)
        const uint32_t classSets = f.tilePerSample ? (uint32_t)B : 1u;       // one classification per camera / scene version
        HIPC(ctx->tileClass.ensure((size_t)genWaves * classSets));
        with_flag(b.multiVer, [&](auto VER) { launch(k_classify_tiles<VER>, dim3((genWaves + 255) / 256, classSets), dim3(256), 0, st, s, f, ctx->tileClass.as<uint8_t>(), tilesX, tilesY); });
        b.tileClass = ctx->tileClass.as<uint8_t>();
    }
    const int genMax = std::min(16, std::max(1, ctx->opt.genGroupMax)), genGroups = (B + genMax - 1) / genMax, genPer = (B + genGroups - 1) / genGroups;     // pixel-major: the batch in equal groups of at most 16 samples, one wave per sample
    const dim3 genGrid = f.genPixelMajor ? dim3(genGroups, genWaves) : dim3(B, (genWaves + 15) / 16), genBlock = f.genPixelMajor ? dim3(64 * genPer) : dim3(1024);
    with_flag(b.multiVer, [&](auto VER) { launch(k_gen_primary<VER>, genGrid, genBlock, 0, st, s, f, b.rays, b.tr, cull, b.activeList, b.activeCount, b.keysTmp, contFlag, b.tileClass, lean); });
    TRACE_T0();
    const bool known = ctx->lastFast && ctx->lastBatch == B;            // the previous batch had this batch's shape: its counts predict this one's
    uint32_t grid0 = b.traceGrid;
    if (ctx->opt.gridRaysX4 > 0 && known) grid0 = small_launch_grid(b.traceGrid, ctx->hCounts[MAX_DEPTH_SLOTS - 1], 2, ctx->opt.gridRaysX4, b.midGrid);
    // fused: FirstHit's traversal, its shading and the bounce's traversal in one persistent launch (kernels_trace_fused.hpp); the bounce's hits are stored per ray id
    if (b.plan.fused) launch(k_trace_fused<32>, dim3(grid0), dim3(WAVE), b.plan.ldsBytes, st, s, f, b.rays, b.tr, b.hits, b.activeList, b.activeCount, b.work + 0, contFlag, b.keysTmp, lean);
    else launch_trace2<true>(ctx, b.plan, grid0, st, s, f, b.rays, b.tr, b.hits, b.activeList, b.activeCount, b.work + 0, b.counters, want_split(ctx, ctx->hCounts[MAX_DEPTH_SLOTS - 1], known, B), 0);
    TRACE_T1();
    if (ctx->capturePrimary) { HIPC(ctx->primHit.ensure((size_t)N * 16)); launch(k_capture_primary, dim3((N + 255) / 256), dim3(256), 0, st, b.hits, (size_t)(B - 1) * b.Npad, N, ctx->primHit.as<float4>()); }
    if (!b.plan.fused) {
        // the first bounce in the primary list's pixel-major order (kernels_shade.hpp k_shade_first): its own work list, hits per ray id
        // (only on sparse views — fewer than half of the pixels entered the traversal in the previous batch of this shape, the pooled leaf phase's rule: measured +1.1 % / +2.2 % on
        // the headline view with 32 / 20 samples in flight, and -1.9 % / -2.3 % where every pixel traverses: the alive queue's runs of 64 neighbouring pixels are coherent there already,
        // and this list is in the order the workgroups happened to append; option bounce_pixel_major: 0 never, 1 sparse views, 2 always)
        const bool sparseView = ctx->lastFast && ctx->lastBatch >= 1 && few_traversed(ctx, ctx->hCounts[MAX_DEPTH_SLOTS - 1], ctx->lastBatch);   // (per sample: the previous batch may have had another size — a warm-up)
        b.pmBounce = f.genPixelMajor && (ctx->opt.bouncePixelMajor >= 2 || (ctx->opt.bouncePixelMajor == 1 && sparseView)) && b.depth >= 2 && !b.multiVer;
        if (b.pmBounce) { HIPC(ctx->pmList.ensure((size_t)b.total * 4)); b.pmList = ctx->pmList.as<uint32_t>(); }
        with_flag(b.multiVer, [&](auto VER) { launch(k_shade_first<VER>, dim3(b.gridTotal), dim3(256), 0, st, s, f, b.rays, b.tr, b.hits, b.activeList, b.activeCount, contFlag, b.keysTmp, lean, b.pmList, VER ? nullptr : b.pmCount); });
    }
    launch(k_scan_local<true>, dim3(b.scanBlocks), dim3(SCAN_WAVES_PER_BLOCK), 0, st, nullptr, b.total, contFlag, b.contMask, b.waveLocal, b.blockSums);
    return first_hit_compact(b);
}

// FirstHit on the generic path (several instances with UseTlas off and no own walk, the debug view, force_generic): one sample, thread-per-ray kernels
static int first_hit_generic(Batch& b)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st; const uint32_t N = b.N;
    TRACE_T0();
    const uint32_t g = std::min<uint32_t>(b.traceGrid, (N + 63) / 64);
    with_flags(ctx->counters, b.debug, [&](auto COUNT, auto COST) { launch(k_trace_primary<COUNT, COST>, dim3(g), dim3(WAVE), b.plan.ldsBytes, st, b.s, b.f, b.rays, b.hits, N, b.work + 0, b.counters); });
    TRACE_T1();
    if (ctx->capturePrimary) { HIPC(ctx->primHit.ensure((size_t)N * 16)); launch(k_capture_primary, dim3((N + 255) / 256), dim3(256), 0, st, b.hits, 0, N, ctx->primHit.as<float4>()); }
    launch(k_shade<true, false>, dim3(b.gridTotal), dim3(256), 0, st, b.s, b.f, b.rays, b.trNone, b.hits, nullptr, nullptr, b.total, nullptr, nullptr, b.contMask, b.waveLocal, b.keysTmp);
    launch(k_scan_local<false>, dim3(b.scanBlocks), dim3(SCAN_WAVES_PER_BLOCK), 0, st, nullptr, b.total, nullptr, b.contMask, b.waveLocal, b.blockSums);
    return first_hit_compact(b);
}

// Exact multi-GPU deep paths: tells every sample of bounce j how many alive rays the contexts above this strip hold (idkpt.h).  gbase: null on a single context;
// f.gbStride / f.gbBands say how k_shade indexes it.
static int exchange_bases(Batch& b, int j, const uint32_t* q, const uint32_t*& gbase)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st; Frame& f = b.f; const int B = b.B;
    gbase = nullptr; f.gbStride = 1; f.gbBands = 0;
    const bool bandExchange = (ctx->bandExchangeFn || ctx->bandExchangeDevFn) && ctx->rowMod > 1 && !(ctx->st.DoRaySorting && j > 1);   // (a member of a multi-device context with interleaved rows takes this route as well)
    if (!bandExchange && ctx->groupExchange) {   // member of a multi-device context: the group sums the counts of the members that own earlier rows, on the device (idkpt_api.hpp)
        const int rc = ctx->groupExchange(ctx->groupUser, ctx, j, B, &gbase); if (rc) ctx->pending.clear(); return rc; }
    if (!bandExchange && ctx->exchangeFn) {
        std::vector<uint32_t> hb(B + 1), local(B), outBases(B, 0u);
        HIPC(hipMemcpyAsync(hb.data(), b.bases + j * BS, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, st)); HIPC(hipStreamSynchronize(st));
        for (int b2 = 0; b2 < B; b2++) local[b2] = hb[b2 + 1] - hb[b2];
        ctx->exchangeFn(ctx->exchangeUser, j, B, local.data(), outBases.data());
        HIPC(ctx->gbases.ensure((size_t)MAX_BATCH * 4));
        HIPC(hipMemcpyAsync(ctx->gbases.p, outBases.data(), (size_t)B * 4, hipMemcpyHostToDevice, st)); HIPC(hipStreamSynchronize(st));                      // outBases is a stack vector
        gbase = ctx->gbases.as<uint32_t>();
    }
    if (!bandExchange) return IDKPT_OK;
    // interleaved rows / bands (idkpt.h idkptSetBandExchange): the rays of one local band are a contiguous run of a sample's queue segment (ordered compaction);
    // the host returns, per (sample, band), the alive rays of all contexts in the image bands before it; k_shade adds the position inside the run
    const int bandRows = 1 << ctx->rowBandLog2, LB = (ctx->rows + bandRows - 1) / bandRows;
    HIPC(ctx->bandTab.ensure((size_t)4 * MAX_BATCH * ((size_t)LB + 1) * 4));
    uint32_t* dStarts = ctx->bandTab.as<uint32_t>(); uint32_t* dTab = dStarts + (size_t)MAX_BATCH * (LB + 1);
    launch(k_band_starts, dim3((uint32_t)(((size_t)B * (LB + 1) + 255) / 256)), dim3(256), 0, st, q, b.bases + j * BS, B, LB, (uint32_t)ctx->W * (uint32_t)bandRows, b.Npad, dStarts);
    if (ctx->bandExchangeDevFn) {
        // device-side variant: counts -> (the host enqueues its exchange on this stream) -> bases -> table; nothing waits on the host
        uint32_t* dCounts = dTab + (size_t)MAX_BATCH * (LB + 1); uint32_t* dBases = dCounts + (size_t)MAX_BATCH * (LB + 1);
        const uint32_t nb = (uint32_t)(((size_t)B * LB + 255) / 256);
        launch(k_band_counts, dim3(nb), dim3(256), 0, st, dStarts, B, LB, dCounts);
        HIPC(hipGetLastError());
        ctx->bandExchangeDevFn(ctx->bandExchangeDevUser, j, B, LB, dCounts, dBases, (void*)st);
        launch(k_band_tab, dim3(nb), dim3(256), 0, st, dStarts, dBases, B, LB, dTab);
    } else {
        std::vector<uint32_t> starts((size_t)B * (LB + 1)), local((size_t)B * LB), outBases((size_t)B * LB, 0u), tab((size_t)B * LB);
        HIPC(hipMemcpyAsync(starts.data(), dStarts, starts.size() * 4, hipMemcpyDeviceToHost, st)); HIPC(hipStreamSynchronize(st));
        for (int k2 = 0; k2 < B; k2++) for (int b2 = 0; b2 < LB; b2++) local[(size_t)k2 * LB + b2] = starts[(size_t)k2 * (LB + 1) + b2 + 1] - starts[(size_t)k2 * (LB + 1) + b2];
        ctx->bandExchangeFn(ctx->bandExchangeUser, j, B, LB, local.data(), outBases.data());
        for (int k2 = 0; k2 < B; k2++) for (int b2 = 0; b2 < LB; b2++) tab[(size_t)k2 * LB + b2] = outBases[(size_t)k2 * LB + b2] - starts[(size_t)k2 * (LB + 1) + b2];   // (mod 2^32: + position inside the sample's segment = global slot)
        HIPC(hipMemcpyAsync(dTab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st)); HIPC(hipStreamSynchronize(st));                      // tab is a stack vector
    }
    gbase = dTab; f.gbStride = LB; f.gbBands = 1;
    return IDKPT_OK;
}

// RaySorting() (PathTracer.cs:232-237): stable sort of (key, rayIndex); key = 21-bit triangle id with the batch's
// sample index above it, so one sort orders every sample's queue exactly like a stand-alone counting sort
static int sort_queue(Batch& b, uint32_t* q, uint32_t* k, const uint32_t* cnt)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st;
    const uint32_t nTiles = (b.total + SORT_TILE - 1) / SORT_TILE;
    int sampleBits = 0; while ((1 << sampleBits) < b.B) sampleBits++;
    const int passes = (IDKPT_SORT_KEY_BITS + sampleBits + 6) / 7;    // 7-bit digits over key + sample index: 3 passes alone, 4 up to 128 samples, 5 up to 256
    uint32_t* hist = ctx->sortHist.as<uint32_t>(); uint32_t* digitTotals = hist + (size_t)SORT_RADIX * nTiles;   // 128 words behind the [digit][tile] table
    uint32_t* ka = k; uint32_t* va = q; uint32_t* kb = ctx->sortKeys.as<uint32_t>(); uint32_t* vb = ctx->sortVals.as<uint32_t>();
    for (int pass = 0; pass < passes; pass++) {
        launch(k_sort_hist, dim3(nTiles), dim3(SORT_BLOCK), 0, st, ka, cnt, (uint32_t)(7 * pass), hist, nTiles);
        launch(k_sort_scan, dim3(SORT_RADIX), dim3(1024), 0, st, cnt, hist, nTiles, digitTotals);
        launch(k_sort_scatter, dim3(nTiles), dim3(SORT_BLOCK), 0, st, ka, va, cnt, (uint32_t)(7 * pass), hist, nTiles, digitTotals, kb, vb);
        std::swap(ka, kb); std::swap(va, vb);
    }
    // odd pass count: the sorted data sits in (sortKeys, sortVals) -> copy the indices back (the reference copies W*H*4 B too, PathTracer.cs:296)
    if (va != q) HIPC(hipMemcpyAsync(q, va, (size_t)b.total * 4, hipMemcpyDeviceToDevice, st));
    return IDKPT_OK;
}

// The traversal launch of bounce j.  Its grid: the queue length is only known on the device; the length the same bounce had in the previous batch (pinned copy,
// possibly one batch stale) is a good predictor, and a grid that is too small or too large only costs time (the waves are persistent)
// readsOnlyHitOrMiss: nothing but hit-or-miss of this launch's records is read (flush_batch); returns whether the launch was the hit-or-miss one (want_occlusion)
// ... and then, with fold_last, the folded one (want_fold): b.f.foldLast is set for it and for the kernels behind it, and the launch is a PRIMARY one — the miss bytes are per ray id, and
// so are the hit records of the rays that keep their closest hit.  Over the alive queue where the bounce has no list of its own: a list of ray ids like any other (b.f.hitsByRid follows)
static bool trace_bounce(Batch& b, int j, const uint32_t* q, const uint32_t* cnt, bool readsOnlyHitOrMiss)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st; const int B = b.B;
    TRACE_T0();
    const bool known = ctx->lastFast && ctx->lastBatch == B && ctx->hBases != nullptr; const uint32_t prev = ctx->hBases ? ctx->hBases[(size_t)j * BS + B] : 0u;
    uint32_t gridj = b.traceGrid;
    const bool split = want_split(ctx, prev, known, B), occl = b.fast && want_occlusion(ctx, b.plan, readsOnlyHitOrMiss, split);
    if (occl) ctx->occlLaunches++;
    if (want_fold(ctx, occl)) { b.f.foldLast = 1; b.f.hitsByRid = 1; }
    if (ctx->opt.gridHint > 0 && ctx->lastBatch == B && ctx->hBases) gridj = small_launch_grid(b.traceGrid, ctx->hBases[(size_t)j * BS + B], ctx->opt.gridHint, ctx->opt.gridRaysX4, b.midGrid);
    if (b.fast && ((b.pmBounce && j == 1) || b.f.foldLast)) {   // the list k_shade_first wrote: ray ids, hits stored per ray id (the PRIMARY instantiations read exactly that); folded: or the alive queue
        const bool pm = b.pmBounce && j == 1;
        Frame ft = b.f; ft.hitsByRid = 0;
        launch_trace2<true>(ctx, b.plan, gridj, st, b.s, ft, b.rays, b.tr, b.hits, pm ? b.pmList : q, pm ? b.pmCount : cnt, b.work + j, b.counters, split, j, occl);
    } else if (b.fast) launch_trace2<false>(ctx, b.plan, gridj, st, b.s, b.f, b.rays, b.tr, b.hits, q, cnt, b.work + j, b.counters, split, j, occl);
    else with_flag(ctx->counters, [&](auto COUNT) { launch(k_trace_queue<COUNT>, dim3(b.traceGrid), dim3(WAVE), b.plan.ldsBytes, st, b.s, b.f, b.rays, b.hits, q, cnt, b.work + j, b.counters); });
    TRACE_T1();
    return occl;
}

// The last bounce where only its radiance is visible in the frame (kernels_shade.hpp k_shade_last): state, queue and counts follow on demand (finish_deferred)
// occl: its traversal launch was the hit-or-miss one — finish_deferred traces the closest hits first
static int defer_last_bounce(Batch& b, int j, const uint32_t* q, const uint32_t* cnt, bool allHits, bool occl)
{
    dev_ctx* ctx = b.ctx;
    const bool fold = b.f.foldLast != 0, pm = b.pmBounce && j == 1;    // (fold: trace_bounce's decision, want_fold — the launch before this call was made for it)
    HIPC(ctx->radSave.ensure((size_t)ctx->maxBatch * ctx->Npad * 16));
    auto shade_last = [&](auto ALL, auto VER) { launch(k_shade_last<ALL, VER>, dim3(b.gridTotal), dim3(256), 0, b.st, b.s, b.f, b.rays, b.hits, q, cnt, b.bases + j * BS, ctx->radSave.as<float4>(), ctx->deferCount.as<uint32_t>()); };
    // folded: the rays left to k_shade_last are the ones write_trace_ready counted (throughput not finite) — a small fixed grid that strides over the queue if there are any
    if (fold) launch(k_shade_last_odd, dim3(std::min<uint32_t>(b.gridTotal, 256u)), dim3(256), 0, b.st, b.s, b.f, b.rays, b.hits, q, cnt, b.bases + j * BS, ctx->radSave.as<float4>(), ctx->deferCount.as<uint32_t>(), (const uint32_t*)b.tr.oddCount);
    else if (allHits) with_flag(b.multiVer, [&](auto VER) { shade_last(std::true_type{}, VER); });
    else shade_last(std::false_type{}, std::false_type{});            // (misses only: the sky is not versioned)
    if (fold) ctx->foldBatches++;
    ctx->defer.allHits = allHits; ctx->defer.valid = true; ctx->defer.j = j; ctx->defer.side = b.side; ctx->defer.B = b.B; ctx->defer.total = b.total; ctx->defer.Npad = b.Npad;
    ctx->defer.occl = occl; ctx->defer.fold = fold; ctx->defer.pm = pm || fold; ctx->defer.list = pm ? (const uint32_t*)b.pmList : q; ctx->defer.ldsBytes = b.plan.ldsBytes; ctx->defer.grid = b.traceGrid;
    return IDKPT_OK;
}

// FinalDraw (which also resets the batch counters for the next batch) and what the context remembers of the batch
static int final_draw(Batch& b)
{
    dev_ctx* ctx = b.ctx; hipStream_t st = b.st;
    ctx->lastQueueSide = b.side; ctx->lastQueueCountSlot = b.depth; ctx->lastFast = b.fast; ctx->lastNeedsRegen = b.fast; ctx->lastTileClass = b.tileClass != nullptr; ctx->lastBatch = b.B; ctx->lastFrame = b.f;
    if (ctx->noiseOn) {                                  // idkptSetNoiseEstimate: the sibling kernel folds the luminance moments in the same loop (one device, whole frame: host_noise.hpp)
        launch(k_final_draw_noise, dim3((b.N + 255) / 256), dim3(256), 0, st, b.s, b.f, b.rays, image_ptr(ctx, 0, 0), image_ptr(ctx, 1, 0), image_ptr(ctx, 2, 0), b.N, b.tileClass, b.work, (uint32_t)WORK_WORDS, b.counts, (uint32_t)MAX_DEPTH_SLOTS, b.tr.oddCount,
               noise_moments_ptr(ctx, 0), noise_mom_stride(ctx));
    } else
    launch(k_final_draw, dim3((b.N + 255) / 256), dim3(256), 0, st, b.s, b.f, b.rays, image_ptr(ctx, 0, 0), image_ptr(ctx, 1, 0), image_ptr(ctx, 2, 0), b.N, b.tileClass, b.work, (uint32_t)WORK_WORDS, b.counts, (uint32_t)MAX_DEPTH_SLOTS, b.tr.oddCount);
    HIPC(hipGetLastError()); ctx->countersDirty = false;
    graph_probe_end(b);
    // queue lengths stay on the GPU during the batch; k_scan_blocks mirrors them into host-mapped memory for GetStats and the queue downloads (no copy, no sync here)
    if (ctx->timing) HIPC(hipEventRecord(ctx->evFrame[1], st));
    ctx->stats.Frames += (uint64_t)b.B; ctx->stats.PrimaryRays += (uint64_t)b.N * (uint64_t)b.B;
    ctx->pending.clear();
    return IDKPT_OK;
}

// One batch of B deferred samples: FirstHit -> [sort ->] NHit x (RayDepth-1) -> FinalDraw (PathTracer.cs:218-270), every
// stage launched once for all B samples.  Sample k owns ray ids [k*Npad, k*Npad+N); alive queues are batch-wide but stay
// grouped by sample (stable compaction / sort with the sample index above the key), and every ray's NHit slot is its
// position inside its own sample's queue, so each sample gets exactly the RNG streams of a stand-alone frame.
static int flush_batch(dev_ctx* ctx)
{
    if (ctx->pending.empty()) return IDKPT_OK;
    if (ctx->grouped && !ctx->inGroupFlush) return fail(ctx, IDKPT_ERR_UNKNOWN, "internal: a member of a multi-device context was flushed on its own");
    if (ctx->noiseOn) { int rc = noise_moments_ensure(ctx); if (rc) return rc; }   // (the moments images FinalDraw folds into: allocated and zeroed at their first batch)
    Batch b; batch_views(ctx, b, (int)ctx->pending.size(), ctx->Npad); int rc;
    if ((rc = stage_versions_cameras(b))) return rc;
    if ((rc = frame_setup(b))) return rc;
    // may the last bounce's continuation wait until somebody asks for it?  (k_shade_last: only where a hit of that bounce cannot change the radiance and nothing else of it reaches the frame)
    const bool deferLast = b.fast && b.depth >= 2 && ctx->opt.deferLast != 0 && !b.f.outputAovs && !b.debug;
    const bool deferAllHits = !(ctx->sceneNoEmission && !(b.f.g.DoTraceLights && b.s.lightCount > 0));   // a hit of the last bounce may add radiance: emission somewhere in the scene, or light hits
    const bool mayFold = may_fold(ctx, deferLast, deferAllHits);
    b.f.markLast = (mayFold && b.depth == 2) ? 1 : 0;                     // (what FirstHit's shading lets continue enters bounce 1)
    if ((rc = b.fast ? first_hit_fast(b) : first_hit_generic(b))) return rc;
    for (int j = 1; j < b.depth; j++) {
        uint32_t* q = ctx->queue[b.side].as<uint32_t>(); uint32_t* k = ctx->keys[b.side].as<uint32_t>();
        const uint32_t* cnt = b.counts + j; const uint32_t* gbase;
        b.f.hitsByRid = (b.plan.fused || (b.pmBounce && j == 1)) ? 1 : 0;     // how this bounce's hit records are indexed (what its shading kernels are told)
        if ((rc = exchange_bases(b, j, q, gbase))) return rc;
        if (ctx->st.DoRaySorting && j > 1) if ((rc = sort_queue(b, q, k, cnt))) return rc;
        // (the deferred last bounce of a scene without emission or light hits — only hit-or-miss of its records is read — may be traced hit-or-miss: want_occlusion holds the whole rule)
        const bool deferThis = deferLast && j == b.depth - 1 && gbase == nullptr;
        bool tookOccl = false;
        if (!b.plan.fused) tookOccl = trace_bounce(b, j, q, cnt, deferThis && !deferAllHits);
        if (deferThis) { if ((rc = defer_last_bounce(b, j, q, cnt, deferAllHits, tookOccl))) return rc; break; }
        b.f.markLast = (mayFold && j + 1 == b.depth - 1) ? 1 : 0;         // (this tail's continuing rays enter bounce j + 1)
        if ((rc = bounce_tail(b, j, q, cnt, gbase, (unsigned long long*)(j + 1 < b.depth ? b.counters + 2 : nullptr), ctx->evBounce != nullptr, b.fast ? b.tr : b.trNone))) return rc;
        b.side = 1 - b.side;
    }
    return final_draw(b);
}


static int32_t dev_Render(dev_ctx* ctx)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    if (!ctx->haveScene) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptRender: no scene uploaded");
    if (ctx->W <= 0 || !ctx->frameOk) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptRender: no frame buffers (idkptSetSize not called, or its allocation failed)");
    if (ctx->st.UseTlas && ctx->tlasCount == 0) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptRender: UseTlas set but no TLAS nodes uploaded");
    HIPC(hipSetDevice(ctx->device));
    if (ctx->timing && ctx->evUsed > 4096) { HIPC(hipStreamSynchronize(ctx->stream)); resolve_trace_events(ctx); }
    // every sample is deferred; a batch is launched as soon as maxBatch samples are pending (or on any call that needs
    // results).  The general path (multi-instance / TLAS / debug cost) is launched sample by sample.
    const int limit = fast_path(ctx) ? ctx->maxBatch : 1;
    for (int i = 0; i < ctx->st.SamplesPerPixel; i++) {
        PendingSample ps; ps.accum = ctx->accum[ctx->curSlot]++; ps.slot = ctx->curSlot;
        memcpy(ps.cam, ctx->invProj, 64); memcpy(ps.cam + 16, ctx->invView, 64); memcpy(ps.cam + 32, ctx->viewPos, 12); ps.cam[35] = 0.0f;
        for (int b = 0; b < VB_COUNT; b++) ps.vs[b] = (uint8_t)ctx->vcur[b];           // the state of the geometry this sample sees
        ctx->pending.push_back(ps);
        if (!ctx->grouped && (int)ctx->pending.size() >= limit) { int rc = flush_batch(ctx); if (rc) return rc; }   // (members of a multi-device context: the group launches)
    }
    return IDKPT_OK;
}

static int32_t dev_Synchronize(dev_ctx* ctx) { if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT; HIPC(hipSetDevice(ctx->device)); FLUSH_KEEP(); SYNC_CHECKED(); return IDKPT_OK; }

// Launches whatever is pending without waiting for it (lets a host overlap its own work with the GPU).
static int32_t dev_Flush(dev_ctx* ctx) { if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT; HIPC(hipSetDevice(ctx->device)); FLUSH_KEEP(); return IDKPT_OK; }

static int32_t dev_SetMaxBatch(dev_ctx* ctx, int32_t maxBatch)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(maxBatch >= 1 && maxBatch <= MAX_BATCH, "idkptSetMaxBatch: 1..256");
    HIPC(hipSetDevice(ctx->device));
    FLUSH();   // (the wavefront buffers are about to be reallocated: a deferred last bounce is completed first)
    HIPC(hipStreamSynchronize(ctx->stream));
    if (maxBatch == ctx->maxBatch) return IDKPT_OK;
    const int previous = ctx->maxBatch;
    ctx->maxBatch = maxBatch;
    if (ctx->W > 0) {
        std::vector<uint32_t> acc = ctx->accum; int slot = ctx->curSlot; const bool started = ctx->ringStarted;
        int rc = alloc_frame_keep_images(ctx);
        if (rc) {   // e.g. out of device memory: fall back to the previous (smaller) buffer set; the accumulation restarts
            const std::string why = ctx->lastError;
            ctx->maxBatch = previous;
            (void)alloc_frame(ctx);
            return fail(ctx, rc, "idkptSetMaxBatch: could not allocate the wavefront buffers for " + std::to_string(maxBatch) + " samples in flight (" + why + "); kept " + std::to_string(previous));
        }
        ctx->accum = acc; ctx->curSlot = slot; ctx->ringStarted = started;
    }
    return IDKPT_OK;
}

// idkptSetSceneVersions: how many states of the geometry may be in flight (1: a scene update launches every queued sample first, as the reference's frame loop does)
static int32_t dev_SetSceneVersions(dev_ctx* ctx, int32_t versions)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(versions >= 1 && versions <= 64, "idkptSetSceneVersions: 1..64 versions");
    HIPC(hipSetDevice(ctx->device));
    if (versions == ctx->verSlots) return IDKPT_OK;
    FLUSH();                                                           // nothing queued or deferred: every buffer has exactly one live state, its current one
    if (versions < ctx->verSlots) {
        for (int b = 0; b < VB_COUNT; b++) {
            if (ctx->vcur[b] >= versions && ctx->vbytes[b] > 0) { HIPC(hipMemcpyAsync(vb_ptr(ctx, b, 0), vb_ptr(ctx, b, ctx->vcur[b]), ctx->vbytes[b], hipMemcpyDeviceToDevice, ctx->stream)); ctx->vcur[b] = 0; }
            ctx->valloc[b] = std::min(ctx->valloc[b], versions);
        }
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    ctx->verSlots = versions;
    return IDKPT_OK;
}

static int32_t dev_SetFrameRing(dev_ctx* ctx, int32_t frames)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(frames >= 1 && frames <= 128, "idkptSetFrameRing: 1..128 frames");
    HIPC(hipSetDevice(ctx->device));
    FLUSH();   // (the wavefront buffers are about to be reallocated: a deferred last bounce is completed first)
    HIPC(hipStreamSynchronize(ctx->stream));
    if (frames == ctx->ringSize) return IDKPT_OK;
    ctx->ringSize = frames;
    if (ctx->W > 0) return alloc_frame(ctx);       // images are re-created (cleared); accumulation restarts in slot 0
    ctx->accum.assign(frames, 0u); ctx->curSlot = 0; ctx->ringStarted = false;
    return IDKPT_OK;
}

static int32_t dev_BeginFrame(dev_ctx* ctx, int32_t* outSlot)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    if (ctx->ringStarted) ctx->curSlot = (ctx->curSlot + 1) % ctx->ringSize;   // the first frame after idkptSetFrameRing / idkptSetSize uses slot 0
    ctx->ringStarted = true;
    ctx->accum[ctx->curSlot] = 0;                   // a new frame: its first sample overwrites whatever the slot held
    if (outSlot) *outSlot = ctx->curSlot;
    return IDKPT_OK;
}
