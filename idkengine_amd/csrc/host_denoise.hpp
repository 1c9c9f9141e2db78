// host_denoise.hpp — idkptDenoise / idkptUploadDenoised / idkptDownloadDenoised / idkptGetDenoisedDevicePtr / idkptGetDenoiseRoute / idkptSetResultSource: the denoised
// image of a ring slot (kernels: kernels_denoise.hpp; the contract: include/idkpt.h), and the driver the three a-trous filters share (denoise_check, denoise_begin,
// denoise_iterate, denoise_ladder).  Part of the single translation unit idkpt.hip (included there, in this order).
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

// ---- the driver of the calls that fill a DenoiseSlot by a-trous iterations: idkptDenoise below, idkptDenoiseVariance (host_denoise_variance.hpp), idkptDenoiseTemporal
// (host_denoise_temporal.hpp).  A filter is: denoise_check, what else it refuses, denoise_begin, its Params, denoise_iterate with a callable that launches one iteration.
// The checks in the order every filter refuses.  The filter judges its own arguments and hands over the message of those that failed (nullptr: none): ownBefore for the
// ones checked before DemodulateAlbedo (its sigmas), ownAfter for the ones behind it.
static int32_t denoise_check(dev_ctx* ctx, const std::string& who, int32_t slot, int32_t iterations, int32_t demodulate, const char* ownBefore, const char* ownAfter = nullptr)
{
    REQUIRE(slot >= -1 && slot < ctx->ringSize, who + ": slot outside the frame ring (-1: the current slot)");
    REQUIRE(iterations >= 1 && iterations <= denoiset::MAX_ITERATIONS, who + ": Iterations must be 1..8");
    REQUIRE(!ownBefore, who + ownBefore);
    REQUIRE(demodulate == 0 || demodulate == 1, who + ": DemodulateAlbedo must be 0 or 1");
    REQUIRE(!ownAfter, who + ownAfter);
    { int rc = denoise_scope(ctx, who.c_str()); if (rc) return rc; }
    if (!ctx->st.OutputAOVs) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, who + ": the current settings have OutputAOVs = 0: the albedo and normal images that guide the filter are not accumulated");
    return IDKPT_OK;
}
// the record of a slot whose denoised image is about to be made (by a filter, an upload or idkptUseTemporalAsDenoised): it holds none until its maker says so
static DenoiseSlot& denoise_slot_invalidated(dev_ctx* ctx, int32_t slot) { DenoiseSlot& s = FrameProducts::slot(ctx->products.denoise, ctx->ringSize, slot); s.valid = false; s.iterations = 0; return s; }

struct DenoiseFill { DenoiseSlot* s; int W, H, n; const float4* albedo; const float4* normal; dim3 grid; };   // what denoise_begin hands over: the slot, the guides, a workgroup per 16 x 16 tile
// Queued samples are launched, `between` (or nullptr) runs, the slot is invalidated and its images are made.  Iteration i writes ping[i & 1] and the last one `out`: ping[0]
// is needed from 2 iterations on, ping[1] from 3 — or always, where the image the first iteration reads lives in ping[1] (firstInPing1: a pre-pass of the filter makes it).
static int32_t denoise_begin(dev_ctx* ctx, int32_t slot, int n, bool firstInPing1, int (*between)(dev_ctx*), DenoiseFill* f)
{
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptBloom)
    { int rc = check_overflow(ctx); if (rc) return rc; }   // (no wait: see idkptGetFrameDevicePtr)
    if (between) { int rc = between(ctx); if (rc) return rc; }
    f->W = ctx->W; f->H = ctx->H; f->n = n; f->s = &denoise_slot_invalidated(ctx, slot);
    const size_t bytes = (size_t)f->W * f->H * 16;
    HIPC(f->s->out.ensure(ctx->stream, bytes));
    if (n >= 2) HIPC(f->s->ping[0].ensure(ctx->stream, bytes));
    if (n >= 3 || firstInPing1) HIPC(f->s->ping[1].ensure(ctx->stream, bytes));
    f->albedo = image_ptr(ctx, IDKPT_IMAGE_ALBEDO, slot); f->normal = image_ptr(ctx, IDKPT_IMAGE_NORMAL, slot);
    f->grid = dim3((unsigned)((f->W + denoisek::TILE - 1) / denoisek::TILE), (unsigned)((f->H + denoisek::TILE - 1) / denoisek::TILE));
    return IDKPT_OK;
}
// launch(i, spacing, route, src, dst, first, last) launches iteration i, which reads `src`: the caller's for the first, then the image the previous one wrote
template <class Launch>
static int32_t denoise_iterate(dev_ctx* ctx, const DenoiseFill& f, const float4* src, const Launch& launch)
{
    DenoiseSlot& s = *f.s;
    for (int i = 0, n = f.n; i < n; i++) {
        float4* dst = (i == n - 1 ? s.out : s.ping[i & 1]).as<float4>();
        s.route[i] = (uint8_t)denoise_route(1 << i);
        launch(i, 1 << i, (int)s.route[i], src, dst, i == 0, i == n - 1);
        src = dst;
    }
    HIPC(hipGetLastError());
    s.iterations = f.n; s.valid = true;
    return IDKPT_OK;
}
// the spacing ladder of a kernel family: direct() launches its direct kernel, tile(DenoiseSpacing<S>()) its tiled kernel's instance for spacing S = 1, 2 or 4
template <int S> struct DenoiseSpacing { static constexpr int value = S; };
template <class Tile, class Direct>
static void denoise_ladder(int route, int spacing, const Tile& tile, const Direct& direct)
{
    if (route == IDKPT_DENOISE_ROUTE_DIRECT) direct();
    else if (spacing == 1) tile(DenoiseSpacing<1>());
    else if (spacing == 2) tile(DenoiseSpacing<2>());
    else tile(DenoiseSpacing<4>());
}

static int32_t dev_Denoise(dev_ctx* ctx, int32_t slot, const idkpt_denoise* d)
{
    if (!ctx || !d) return IDKPT_ERR_INVALID_ARGUMENT;
    auto sigma = [](float v) { return v - v == 0.0f && v > 0.0f; };
    const bool sigmas = sigma(d->ColorSigma) && sigma(d->AlbedoSigma) && sigma(d->NormalSigma);
    { int rc = denoise_check(ctx, "idkptDenoise", slot, d->Iterations, d->DemodulateAlbedo, sigmas ? nullptr : ": ColorSigma, AlbedoSigma and NormalSigma must be finite and > 0"); if (rc) return rc; }
    if (slot < 0) slot = ctx->curSlot;
    const bool temporalIn = ctx->denoiseInput == IDKPT_DENOISE_INPUT_TEMPORAL;   // idkptSetDenoiseInput: c0 is the slot's temporal rgb (host_reproject.hpp)
    if (temporalIn && !((size_t)slot < ctx->products.temporal.size() && ctx->products.temporal[slot].temporalValid))
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoise: the denoise input is IDKPT_DENOISE_INPUT_TEMPORAL and the slot holds no temporal image since the last resize (idkptReproject)");
    DenoiseFill f;
    { int rc = denoise_begin(ctx, slot, d->Iterations, false, nullptr, &f); if (rc) return rc; }
    denoisek::Params p;
    p.W = f.W; p.H = f.H; p.invA = denoiset::inv_sigma2(d->AlbedoSigma, 0); p.invN = denoiset::inv_sigma2(d->NormalSigma, 0);
    const float4* c0 = temporalIn ? ctx->products.temporal[slot].temporal.as<const float4>() : image_ptr(ctx, IDKPT_IMAGE_RESULT, slot);
    return denoise_iterate(ctx, f, c0, [&](int i, int spacing, int route, const float4* src, float4* dst, bool first, bool last) {
        p.s = spacing; p.invC = denoiset::inv_sigma2(d->ColorSigma, i);
        p.demodIn = d->DemodulateAlbedo && first; p.remodOut = d->DemodulateAlbedo && last;
        denoise_ladder(route, spacing,
            [&](auto S) { hipLaunchKernelGGL((k_denoise_tile<decltype(S)::value>), f.grid, dim3(256), 0, ctx->stream, src, f.albedo, f.normal, dst, p); },
            [&] { hipLaunchKernelGGL(k_denoise_direct, f.grid, dim3(256), 0, ctx->stream, src, f.albedo, f.normal, dst, p); });
    });
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
    DenoiseSlot& s = denoise_slot_invalidated(ctx, slot);
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
