// host_denoise.hpp — idkptDenoise / idkptUploadDenoised / idkptDownloadDenoised / idkptGetDenoisedDevicePtr / idkptGetDenoiseRoute / idkptSetResultSource: the denoised
// image of a ring slot (kernels: kernels_denoise.hpp; the contract: include/idkpt.h).  Part of the single translation unit idkpt.hip (included there, in this order).
// Queued samples are launched first, nothing but the download waits for the GPU.  A frame product (host_context.hpp, "frame products": the life cycle of the buffers): the
// denoised image and the two images the iterations alternate between, all RGBA32F of the render size.
// One device, the whole frame: the taps of iteration i reach 2 * 2^i rows, a shard of the rows would need halos as tall as that.
#pragma once

static int denoise_route(int spacing) { return spacing <= denoisek::MAX_TILE_SPACING ? IDKPT_DENOISE_ROUTE_TILED : IDKPT_DENOISE_ROUTE_DIRECT; }
// what every call that makes or reads a denoised image needs of the context, after its arguments were checked
static int32_t denoise_scope(dev_ctx* ctx, const char* who)
{
    if (ctx->W <= 0 || !ctx->frameOk) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, std::string(who) + ": no frame buffers (idkptSetSize not called)");
    if (!owns_whole_frame(ctx)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, std::string(who) + ": the context holds a shard of the rows (idkptSetRowSharding / idkptSetRowBands / idkptSetRowRange) or is a member of a multi-device context; the denoised image needs the whole frame on one device");
    return IDKPT_OK;
}
static int32_t dev_Denoise(dev_ctx* ctx, int32_t slot, const idkpt_denoise* d)
{
    if (!ctx || !d) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptDenoise: slot outside the frame ring (-1: the current slot)");
    REQUIRE(d->Iterations >= 1 && d->Iterations <= denoiset::MAX_ITERATIONS, "idkptDenoise: Iterations must be 1..8");
    auto sigma = [](float v) { return v - v == 0.0f && v > 0.0f; };
    REQUIRE(sigma(d->ColorSigma) && sigma(d->AlbedoSigma) && sigma(d->NormalSigma), "idkptDenoise: ColorSigma, AlbedoSigma and NormalSigma must be finite and > 0");
    REQUIRE(d->DemodulateAlbedo == 0 || d->DemodulateAlbedo == 1, "idkptDenoise: DemodulateAlbedo must be 0 or 1");
    { int rc = denoise_scope(ctx, "idkptDenoise"); if (rc) return rc; }
    if (!ctx->st.OutputAOVs) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoise: the current settings have OutputAOVs = 0: the albedo and normal images that guide the filter are not accumulated");
    if (slot < 0) slot = ctx->curSlot;
    const bool temporalIn = ctx->denoiseInput == IDKPT_DENOISE_INPUT_TEMPORAL;   // idkptSetDenoiseInput: c0 is the slot's temporal rgb (host_reproject.hpp)
    if (temporalIn && !((size_t)slot < ctx->products.temporal.size() && ctx->products.temporal[slot].temporalValid))
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoise: the denoise input is IDKPT_DENOISE_INPUT_TEMPORAL and the slot holds no temporal image since the last resize (idkptReproject)");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptBloom)
    { int rc = check_overflow(ctx); if (rc) return rc; }   // (no wait: see idkptGetFrameDevicePtr)
    const int W = ctx->W, H = ctx->H, n = d->Iterations;
    const size_t bytes = (size_t)W * H * 16;
    DenoiseSlot& s = FrameProducts::slot(ctx->products.denoise, ctx->ringSize, slot);
    s.valid = false; s.iterations = 0;
    HIPC(s.out.ensure(ctx->stream, bytes));
    for (int k = 0; k < 2 && k < n - 1; k++) HIPC(s.ping[k].ensure(ctx->stream, bytes));
    const float4* albedo = image_ptr(ctx, IDKPT_IMAGE_ALBEDO, slot); const float4* normal = image_ptr(ctx, IDKPT_IMAGE_NORMAL, slot);
    const dim3 grid((unsigned)((W + denoisek::TILE - 1) / denoisek::TILE), (unsigned)((H + denoisek::TILE - 1) / denoisek::TILE));
    const float4* src = temporalIn ? ctx->products.temporal[slot].temporal.as<const float4>() : image_ptr(ctx, IDKPT_IMAGE_RESULT, slot);
    for (int i = 0; i < n; i++) {
        float4* dst = (i == n - 1 ? s.out : s.ping[i & 1]).as<float4>();
        denoisek::Params p;
        p.W = W; p.H = H; p.s = 1 << i;
        p.invC = denoiset::inv_sigma2(d->ColorSigma, i); p.invA = denoiset::inv_sigma2(d->AlbedoSigma, 0); p.invN = denoiset::inv_sigma2(d->NormalSigma, 0);
        p.demodIn = d->DemodulateAlbedo && i == 0; p.remodOut = d->DemodulateAlbedo && i == n - 1;
        s.route[i] = (uint8_t)denoise_route(p.s);
        if (s.route[i] == IDKPT_DENOISE_ROUTE_DIRECT) hipLaunchKernelGGL(k_denoise_direct, grid, dim3(256), 0, ctx->stream, src, albedo, normal, dst, p);
        else if (p.s == 1) hipLaunchKernelGGL((k_denoise_tile<1>), grid, dim3(256), 0, ctx->stream, src, albedo, normal, dst, p);
        else if (p.s == 2) hipLaunchKernelGGL((k_denoise_tile<2>), grid, dim3(256), 0, ctx->stream, src, albedo, normal, dst, p);
        else hipLaunchKernelGGL((k_denoise_tile<4>), grid, dim3(256), 0, ctx->stream, src, albedo, normal, dst, p);
        src = dst;
    }
    HIPC(hipGetLastError());
    s.iterations = n; s.valid = true;
    return IDKPT_OK;
}

// the host's own denoiser's output (the reference's denoisedTexture.Upload2D): the array is borrowed for the call only and the copy must not make the call wait for the
// stream, so the bytes go through a pinned buffer of the context's own (PinnedUpload: only the PREVIOUS upload's copy is waited for)
static int32_t dev_UploadDenoised(dev_ctx* ctx, int32_t slot, const float* rgba, size_t bytes)
{
    if (!ctx || !rgba) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptUploadDenoised: slot outside the frame ring (-1: the current slot)");
    { int rc = denoise_scope(ctx, "idkptUploadDenoised"); if (rc) return rc; }
    const size_t need = (size_t)ctx->W * ctx->H * 16;
    REQUIRE(bytes == need, "idkptUploadDenoised: bytes must equal height*width*16");
    if (slot < 0) slot = ctx->curSlot;
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();
    DenoiseSlot& s = FrameProducts::slot(ctx->products.denoise, ctx->ringSize, slot);
    s.valid = false; s.iterations = 0;
    HIPC(s.out.ensure(ctx->stream, need));
    HIPC(ctx->denoiseStage.stage(rgba, need));
    HIPC(hipMemcpyAsync(s.out.mem.p, ctx->denoiseStage.host, need, hipMemcpyHostToDevice, ctx->stream));
    HIPC(ctx->denoiseStage.done(ctx->stream));
    s.valid = true;
    return IDKPT_OK;
}

#define DENOISED_NONE ": the slot holds no denoised image since the last resize (idkptDenoise / idkptUploadDenoised)"
static int32_t dev_DownloadDenoised(dev_ctx* ctx, int32_t slot, float* rgba, size_t bytes)
{
    if (!ctx || !rgba) return IDKPT_ERR_INVALID_ARGUMENT;
    DenoiseSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.denoise, "idkptDownloadDenoised", slot, DENOISED_NONE, &s); if (rc) return rc; }
    REQUIRE(bytes == s->out.bytes, "idkptDownloadDenoised: bytes must equal height*width*16");
    return download_behind_queue(ctx, rgba, s->out.mem.p, bytes);
}
static int32_t dev_GetDenoisedDevicePtr(dev_ctx* ctx, int32_t slot, void** outPtr, size_t* outBytes)
{
    if (!ctx || !outPtr) return IDKPT_ERR_INVALID_ARGUMENT;
    DenoiseSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.denoise, "idkptGetDenoisedDevicePtr", slot, DENOISED_NONE, &s); if (rc) return rc; }
    *outPtr = s->out.mem.p;
    if (outBytes) *outBytes = s->out.bytes;
    return IDKPT_OK;
}
static int32_t dev_GetDenoiseRoute(dev_ctx* ctx, int32_t slot, int32_t iteration, int32_t* route)
{
    if (!ctx || !route) return IDKPT_ERR_INVALID_ARGUMENT;
    DenoiseSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.denoise, "idkptGetDenoiseRoute", slot, DENOISED_NONE, &s); if (rc) return rc; }
    REQUIRE(iteration >= 0 && iteration < s->iterations, "idkptGetDenoiseRoute: iteration outside the slot's last idkptDenoise (an uploaded image has none)");
    *route = s->route[iteration];
    return IDKPT_OK;
}

static int32_t dev_SetResultSource(dev_ctx* ctx, int32_t source)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(source == IDKPT_RESULT_NOISY || source == IDKPT_RESULT_DENOISED, "idkptSetResultSource: source must be IDKPT_RESULT_NOISY or IDKPT_RESULT_DENOISED");
    if (source == IDKPT_RESULT_DENOISED && !owns_whole_frame(ctx))
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptSetResultSource: the denoised image needs the whole frame on one device; this context holds a shard of the rows or is a member of a multi-device context");
    ctx->resultSource = source;
    return IDKPT_OK;
}
static int32_t dev_GetResultSource(dev_ctx* ctx, int32_t* out) { if (!ctx || !out) return IDKPT_ERR_INVALID_ARGUMENT; *out = ctx->resultSource; return IDKPT_OK; }
