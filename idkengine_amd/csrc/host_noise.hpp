// host_noise.hpp — idkptSetNoiseEstimate / idkptGetNoiseEstimate / idkptEstimateNoise / idkptDownloadNoise / idkptGetNoiseDevicePtr / idkptDownloadMoments /
// idkptGetMomentsDevicePtr: the luminance moments FinalDraw keeps per pixel while the switch is on, and the per-tile error map made of them (kernels: kernels_frame.hpp
// k_final_draw_noise, kernels_noise.hpp; the contract: include/idkpt.h).  Part of the single translation unit idkpt.hip (included there, in this order).
// Queued samples are launched first, nothing but the downloads waits for the GPU.  A frame product (host_context.hpp, "frame products": the life cycle of the buffers); a
// context that never turns the switch on allocates nothing.  The moments images of all ring slots share one allocation, slot q at q * noise_mom_stride float4s (FinalDraw
// switches slots inside a batch by an offset, as it does for the accumulated images); each slot's guard bytes lie behind its image.
// One device, the whole frame (the scope of idkptDenoise): the switch cannot be turned on elsewhere, and a row-layout call that leaves a shard turns it off.
// (Included in front of host_schedule.hpp: FinalDraw's launch needs the moments images.)
#pragma once

static size_t noise_mom_stride(const dev_ctx* ctx) { return (size_t)ctx->W * ctx->rows + GUARD_BYTES / 16; }   // float4s from one slot's moments image to the next
static size_t noise_mom_bytes(const dev_ctx* ctx) { return (size_t)ctx->W * ctx->rows * 16; }

// the moments images (zeroed, guards written) — FinalDraw's first batch with the switch on, or the first call that reads them
static int noise_moments_ensure(dev_ctx* ctx)
{
    if (ctx->products.moments.p) return IDKPT_OK;                 // (released with every other frame product)
    const size_t stride = noise_mom_stride(ctx) * 16, body = noise_mom_bytes(ctx);
    HIPC(ctx->products.moments.ensure(stride * ctx->ringSize));
    HIPC(hipMemsetAsync(ctx->products.moments.p, 0, stride * ctx->ringSize, ctx->stream));
    for (int q = 0; q < ctx->ringSize; q++) HIPC(hipMemsetAsync((char*)ctx->products.moments.p + q * stride + body, 0xA5, GUARD_BYTES, ctx->stream));
    return IDKPT_OK;
}
static float4* noise_moments_ptr(dev_ctx* ctx, int slot) { return ctx->products.moments.as<float4>() + (size_t)slot * noise_mom_stride(ctx); }

static int32_t dev_SetNoiseEstimate(dev_ctx* ctx, int32_t enable)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(enable == 0 || enable == 1, "idkptSetNoiseEstimate: enable must be 0 or 1");
    if (enable && !owns_whole_frame(ctx))
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptSetNoiseEstimate: the context holds a shard of the rows (idkptSetRowSharding / idkptSetRowBands / idkptSetRowRange) or is a member of a multi-device context; the noise estimate needs the whole frame on one device");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // the queued samples are folded the way they were submitted
    if (enable == ctx->noiseOn) return IDKPT_OK;
    ctx->noiseOn = enable;
    std::fill(ctx->accum.begin(), ctx->accum.end(), 0u);   // moments and images count the same samples: the accumulation starts over (as idkptSetSampleSequence)
    ctx->products.release_noise();                            // off: nothing stays allocated; on: zeroed again at first use
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
    NoiseSlot& s = FrameProducts::slot(ctx->products.noise, ctx->ringSize, slot);
    s.valid = false;
    HIPC(s.tiles.ensure(ctx->stream, (size_t)nTiles * 8));
    HIPC(s.summary.ensure(ctx->stream, sizeof(idkpt_noise_summary)));
    HIPC(hipMemsetAsync(s.summary.mem.p, 0, sizeof(idkpt_noise_summary), ctx->stream));   // TilesAbove = 0, MaxTileMean = +0.0
    hipLaunchKernelGGL(k_noise_estimate, dim3((nTiles + noisek::WAVES - 1) / noisek::WAVES), dim3(256), 0, ctx->stream, (const float4*)noise_moments_ptr(ctx, slot), W, H, n, p->Epsilon, p->Threshold,
                       s.tiles.as<float2>(), s.summary.as<uint32_t>());
    HIPC(hipGetLastError());
    s.tilesX = tilesX; s.tilesY = tilesY; s.valid = true;
    return IDKPT_OK;
}

#define NOISE_NONE ": the slot holds no estimate since the last resize (idkptEstimateNoise)"
static int32_t dev_DownloadNoise(dev_ctx* ctx, int32_t slot, float* tiles, size_t bytes, idkpt_noise_summary* summary)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    NoiseSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.noise, "idkptDownloadNoise", slot, NOISE_NONE, &s); if (rc) return rc; }
    REQUIRE(!tiles || bytes == s->tiles.bytes, "idkptDownloadNoise: bytes must equal tilesX*tilesY*8 (tiles of 8 x 8 pixels, two floats each)");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();
    if (tiles) HIPC(hipMemcpyAsync(tiles, s->tiles.mem.p, s->tiles.bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (summary) HIPC(hipMemcpyAsync(summary, s->summary.mem.p, sizeof(idkpt_noise_summary), hipMemcpyDeviceToHost, ctx->stream));
    SYNC_CHECKED();
    return IDKPT_OK;
}
static int32_t dev_GetNoiseDevicePtr(dev_ctx* ctx, int32_t slot, void** tiles, void** summary, size_t* tileBytes)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    NoiseSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.noise, "idkptGetNoiseDevicePtr", slot, NOISE_NONE, &s); if (rc) return rc; }
    if (tiles) *tiles = s->tiles.mem.p;
    if (summary) *summary = s->summary.mem.p;
    if (tileBytes) *tileBytes = s->tiles.bytes;
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
