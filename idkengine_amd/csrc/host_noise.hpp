// host_noise.hpp — idkptSetNoiseEstimate / idkptGetNoiseEstimate / idkptEstimateNoise / idkptDownloadNoise / idkptGetNoiseDevicePtr / idkptDownloadMoments /
// idkptGetMomentsDevicePtr: the luminance moments FinalDraw keeps per pixel while the switch is on, and the per-tile error map made of them (kernels: kernels_frame.hpp
// k_final_draw_noise, kernels_noise.hpp; the contract: include/idkpt.h).  Part of the single translation unit idkpt.hip (included there, in this order).
// Behaves as idkptDenoise does (host_denoise.hpp): queued samples are launched first, nothing but the downloads waits for the GPU, the buffers belong to a ring slot and a
// frame size, are allocated at first use — a context that never turns the switch on allocates nothing —, released by alloc_frame_impl, kept by idkptSetMaxBatch, and each
// ends with NOISE_GUARD_BYTES of 0xA5 that nothing writes.  The moments images of all ring slots share one allocation, slot q at q * noise_mom_stride float4s (FinalDraw
// switches slots inside a batch by an offset, as it does for the accumulated images); each slot's guard bytes lie behind its image.
// One device, the whole frame (the scope of idkptDenoise): the switch cannot be turned on elsewhere, and a row-layout call that leaves a shard turns it off.
#pragma once

#define NOISE_GUARD_BYTES 64
static size_t noise_mom_stride(const dev_ctx* ctx) { return (size_t)ctx->W * ctx->rows + NOISE_GUARD_BYTES / 16; }   // float4s from one slot's moments image to the next
static size_t noise_mom_bytes(const dev_ctx* ctx) { return (size_t)ctx->W * ctx->rows * 16; }

// the moments images (zeroed, guards written) — FinalDraw's first batch with the switch on, or the first call that reads them
static int noise_moments_ensure(dev_ctx* ctx)
{
    if (ctx->noiseMom.p) return IDKPT_OK;                 // (alloc_frame_impl releases it with everything else that has the frame's size)
    const size_t stride = noise_mom_stride(ctx) * 16, body = noise_mom_bytes(ctx);
    HIPC(ctx->noiseMom.ensure(stride * ctx->ringSize));
    HIPC(hipMemsetAsync(ctx->noiseMom.p, 0, stride * ctx->ringSize, ctx->stream));
    for (int q = 0; q < ctx->ringSize; q++) HIPC(hipMemsetAsync((char*)ctx->noiseMom.p + q * stride + body, 0xA5, NOISE_GUARD_BYTES, ctx->stream));
    return IDKPT_OK;
}
static float4* noise_moments_ptr(dev_ctx* ctx, int slot) { return ctx->noiseMom.as<float4>() + (size_t)slot * noise_mom_stride(ctx); }
static void noise_release(dev_ctx* ctx)
{
    ctx->noiseMom.release();
    for (NoiseSlot& s : ctx->noise) s.release();
    ctx->noise.clear();
}
static NoiseSlot& noise_slot(dev_ctx* ctx, int slot)
{
    if (ctx->noise.size() != (size_t)ctx->ringSize) { for (NoiseSlot& s : ctx->noise) s.release(); ctx->noise.assign(ctx->ringSize, NoiseSlot()); }
    return ctx->noise[slot];
}

static int32_t dev_SetNoiseEstimate(dev_ctx* ctx, int32_t enable)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(enable == 0 || enable == 1, "idkptSetNoiseEstimate: enable must be 0 or 1");
    if (enable && (ctx->grouped || !holds_whole_frame(ctx)))
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptSetNoiseEstimate: the context holds a shard of the rows (idkptSetRowSharding / idkptSetRowBands / idkptSetRowRange) or is a member of a multi-device context; the noise estimate needs the whole frame on one device");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // the queued samples are folded the way they were submitted
    if (enable == ctx->noiseOn) return IDKPT_OK;
    ctx->noiseOn = enable;
    std::fill(ctx->accum.begin(), ctx->accum.end(), 0u);   // moments and images count the same samples: the accumulation starts over (as idkptSetSampleSequence)
    noise_release(ctx);                                  // off: nothing stays allocated; on: zeroed again at first use
    return IDKPT_OK;
}
static int32_t dev_GetNoiseEstimate(dev_ctx* ctx, int32_t* out) { if (!ctx || !out) return IDKPT_ERR_INVALID_ARGUMENT; *out = ctx->noiseOn; return IDKPT_OK; }

// what every call that reads the moments needs of the context, after its arguments were checked
static int32_t noise_scope(dev_ctx* ctx, const char* who)
{
    if (ctx->W <= 0 || !ctx->frameOk) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, std::string(who) + ": no frame buffers (idkptSetSize not called)");
    if (!ctx->noiseOn) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, std::string(who) + ": the noise estimate is off (idkptSetNoiseEstimate): no moments are kept");
    return IDKPT_OK;
}

static int32_t dev_EstimateNoise(dev_ctx* ctx, int32_t slot, const idkpt_noise* p)
{
    if (!ctx || !p) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptEstimateNoise: slot outside the frame ring (-1: the current slot)");
    REQUIRE(noiset::finite(p->Epsilon) && p->Epsilon > 0.0f, "idkptEstimateNoise: Epsilon must be finite and > 0");
    REQUIRE(noiset::finite(p->Threshold) && p->Threshold >= 0.0f, "idkptEstimateNoise: Threshold must be finite and >= 0");
    { int rc = noise_scope(ctx, "idkptEstimateNoise"); if (rc) return rc; }
    if (slot < 0) slot = ctx->curSlot;
    const uint32_t n = ctx->accum[slot];                 // (queued samples included: they are launched below)
    if (n < 2u) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptEstimateNoise: the slot has accumulated fewer than 2 samples: a variance needs two");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptDenoise)
    { int rc = check_overflow(ctx); if (rc) return rc; }   // (no wait: see idkptGetFrameDevicePtr)
    { int rc = noise_moments_ensure(ctx); if (rc) return rc; }
    const int W = ctx->W, H = ctx->H, tilesX = (W + 7) / 8, tilesY = (H + 7) / 8;
    const uint32_t nTiles = (uint32_t)tilesX * (uint32_t)tilesY;
    NoiseSlot& s = noise_slot(ctx, slot);
    s.valid = false;
    { int rc = bloom_ensure(ctx, s.tiles, s.tileBytes, (size_t)nTiles * 8); if (rc) return rc; }
    { int rc = bloom_ensure(ctx, s.summary, s.summaryBytes, sizeof(idkpt_noise_summary)); if (rc) return rc; }
    HIPC(hipMemsetAsync(s.summary.p, 0, sizeof(idkpt_noise_summary), ctx->stream));   // TilesAbove = 0, MaxTileMean = +0.0
    hipLaunchKernelGGL(k_noise_estimate, dim3((nTiles + noisek::WAVES - 1) / noisek::WAVES), dim3(256), 0, ctx->stream, (const float4*)noise_moments_ptr(ctx, slot), W, H, n, p->Epsilon, p->Threshold,
                       s.tiles.as<float2>(), s.summary.as<uint32_t>());
    HIPC(hipGetLastError());
    s.tilesX = tilesX; s.tilesY = tilesY; s.valid = true;
    return IDKPT_OK;
}

// the estimate of a slot; INVALID_OPERATION when the slot holds none since the last resize
static int32_t noise_of(dev_ctx* ctx, const char* who, int32_t slot, NoiseSlot** out)
{
    REQUIRE(slot >= -1 && slot < ctx->ringSize, std::string(who) + ": slot outside the frame ring (-1: the current slot)");
    if (slot < 0) slot = ctx->curSlot;
    if ((size_t)slot >= ctx->noise.size() || !ctx->noise[slot].valid) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, std::string(who) + ": the slot holds no estimate since the last resize (idkptEstimateNoise)");
    *out = &ctx->noise[slot];
    return IDKPT_OK;
}
static int32_t dev_DownloadNoise(dev_ctx* ctx, int32_t slot, float* tiles, size_t bytes, idkpt_noise_summary* summary)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    NoiseSlot* s = nullptr;
    { int rc = noise_of(ctx, "idkptDownloadNoise", slot, &s); if (rc) return rc; }
    REQUIRE(!tiles || bytes == s->tileBytes, "idkptDownloadNoise: bytes must equal tilesX*tilesY*8 (tiles of 8 x 8 pixels, two floats each)");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();
    if (tiles) HIPC(hipMemcpyAsync(tiles, s->tiles.p, s->tileBytes, hipMemcpyDeviceToHost, ctx->stream));
    if (summary) HIPC(hipMemcpyAsync(summary, s->summary.p, sizeof(idkpt_noise_summary), hipMemcpyDeviceToHost, ctx->stream));
    SYNC_CHECKED();
    return IDKPT_OK;
}
static int32_t dev_GetNoiseDevicePtr(dev_ctx* ctx, int32_t slot, void** tiles, void** summary, size_t* tileBytes)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    NoiseSlot* s = nullptr;
    { int rc = noise_of(ctx, "idkptGetNoiseDevicePtr", slot, &s); if (rc) return rc; }
    if (tiles) *tiles = s->tiles.p;
    if (summary) *summary = s->summary.p;
    if (tileBytes) *tileBytes = s->tileBytes;
    return IDKPT_OK;
}

static int32_t dev_DownloadMoments(dev_ctx* ctx, int32_t slot, float* rgba, size_t bytes)
{
    if (!ctx || !rgba) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptDownloadMoments: slot outside the frame ring (-1: the current slot)");
    { int rc = noise_scope(ctx, "idkptDownloadMoments"); if (rc) return rc; }
    REQUIRE(bytes == noise_mom_bytes(ctx), "idkptDownloadMoments: bytes must equal height*width*16");
    if (slot < 0) slot = ctx->curSlot;
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();
    { int rc = noise_moments_ensure(ctx); if (rc) return rc; }
    HIPC(hipMemcpyAsync(rgba, noise_moments_ptr(ctx, slot), bytes, hipMemcpyDeviceToHost, ctx->stream));
    SYNC_CHECKED();
    return IDKPT_OK;
}
static int32_t dev_GetMomentsDevicePtr(dev_ctx* ctx, int32_t slot, void** outPtr, size_t* outBytes)
{
    if (!ctx || !outPtr) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptGetMomentsDevicePtr: slot outside the frame ring (-1: the current slot)");
    { int rc = noise_scope(ctx, "idkptGetMomentsDevicePtr"); if (rc) return rc; }
    if (slot < 0) slot = ctx->curSlot;
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();
    { int rc = noise_moments_ensure(ctx); if (rc) return rc; }
    *outPtr = noise_moments_ptr(ctx, slot);
    if (outBytes) *outBytes = noise_mom_bytes(ctx);
    return IDKPT_OK;
}
