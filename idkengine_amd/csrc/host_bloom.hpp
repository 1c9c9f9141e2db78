// host_bloom.hpp — idkptBloom / idkptGetBloomInfo / idkptDownloadBloom / idkptGetBloomDevicePtr: Bloom.Compute (Source/Render/Bloom.cs:56-127) on the device
// (kernels: kernels_bloom.hpp).  Part of the single translation unit idkpt.hip (included there, in this order).
// Queued samples are launched first, nothing waits for the GPU.  A frame product (host_context.hpp, "frame products": the life cycle of the buffers) with three buffers per
// slot: the down chain, the up chain (RGBA16F levels one behind the other), the expanded RGBA32F image.
// The chain and the expanded image have the presentation size (host_context.hpp pres_w / pres_h; the render size by default), the image they start from the render size.
// One device, the whole frame: bloom is a global filter (the last level mixes the whole image), a shard of the rows would need halos as wide as the chain.
#pragma once

static size_t bloom_level_texels(int w0, int h0, int level) { return (size_t)bloomt::level_dim(w0, level) * (size_t)bloomt::level_dim(h0, level); }
static size_t bloom_level_offset(int w0, int h0, int level) { size_t t = 0; for (int l = 0; l < level; l++) t += bloom_level_texels(w0, h0, l); return t; }   // texels in front of `level`
// k_bloom_down0 stages SRC_TILE source texels per axis: true when every tile of a level of `dsize` texels reading `ssize` texels stays inside
static bool bloom_tile_spans_fit(int dsize, int ssize)
{
    for (int t0 = 0; t0 < dsize; t0 += bloomk::TILE) {
        int lo, hi; bloomk::tap_range(t0, std::min(t0 + bloomk::TILE - 1, dsize - 1), dsize, ssize, 2, &lo, &hi);
        if (hi - lo + 1 > bloomk::SRC_TILE) return false;
    }
    return true;
}

static int32_t dev_Bloom(dev_ctx* ctx, int32_t slot, int32_t image, const idkpt_bloom* b)
{
    if (!ctx || !b) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptBloom: slot outside the frame ring (-1: the current slot)");
    REQUIRE(image >= 0 && image < 3, "idkptBloom: bad image id");
    auto fin = [](float v) { return v - v == 0.0f; };
    REQUIRE(fin(b->Threshold) && fin(b->MaxColor), "idkptBloom: Threshold and MaxColor must be finite");
    REQUIRE(b->MinusLods >= 0, "idkptBloom: MinusLods must not be negative");
    if (ctx->W <= 0 || !ctx->frameOk) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptBloom: no frame buffers (idkptSetSize not called)");
    if (present_scaled(ctx) && !owns_whole_frame(ctx))
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptBloom: a presentation size other than the render size (idkptSetPresentationSize) needs one device that holds the whole frame; this context holds a shard of the rows");
    if (!holds_whole_frame(ctx)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptBloom: the context holds a shard of the rows (idkptSetRowSharding / idkptSetRowBands / idkptSetRowRange); bloom needs the whole frame on one device");
    // the chain is sized from the PRESENTATION size (Bloom.SetSize(presentRes), Application.cs:570-586), which is the render size unless idkptSetPresentationSize said otherwise
    const int W = ctx->W, H = ctx->H, pw = pres_w(ctx), ph = pres_h(ctx);
    if (pw < 2 || ph < 2) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptBloom: the frame must be at least 2 x 2 (level 0 is width / 2 x height / 2)");
    if (slot < 0) slot = ctx->curSlot;
    if (source_missing(ctx, image, slot)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptBloom: the result source is IDKPT_RESULT_DENOISED and the slot holds no denoised image since the last resize (idkptDenoise / idkptUploadDenoised)");
    int w0 = 0, h0 = 0;
    const int levels = bloomt::bloom_levels(pw, ph, b->MinusLods, &w0, &h0);
    // a render size up to the presentation size (and the equal sizes of a context without one) always fits the staged tile; a larger one (supersampling) may not
    const bool direct = !bloom_tile_spans_fit(w0, W) || !bloom_tile_spans_fit(h0, H);
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptPresent)
    { int rc = check_overflow(ctx); if (rc) return rc; }   // (no wait: see idkptGetFrameDevicePtr)
    BloomSlot& s = FrameProducts::slot(ctx->products.bloom, ctx->ringSize, slot);
    s.valid = false;
    HIPC(s.down.ensure(ctx->stream, bloom_level_offset(w0, h0, levels) * 8));
    HIPC(s.up.ensure(ctx->stream, bloom_level_offset(w0, h0, levels - 1) * 8));
    HIPC(s.out.ensure(ctx->stream, (size_t)pw * ph * 16));
    auto lvl = [&](GuardedBuf& buf, int l) { return buf.as<uint2>() + bloom_level_offset(w0, h0, l); };
    auto dim = [](int d0, int l) { return bloomt::level_dim(d0, l); };
    auto grid = [](int w, int h) { return dim3((unsigned)((w + bloomk::TILE - 1) / bloomk::TILE), (unsigned)((h + bloomk::TILE - 1) / bloomk::TILE)); };
    // down pass 0: the image, Lod 0, Prefilter -> down level 0
    if (direct) hipLaunchKernelGGL(k_bloom_down0_direct, grid(w0, h0), dim3(256), 0, ctx->stream, source_ptr(ctx, image, slot), W, H, lvl(s.down, 0), w0, h0, b->MaxColor, b->Threshold);
    else hipLaunchKernelGGL(k_bloom_down0, grid(w0, h0), dim3(256), 0, ctx->stream, source_ptr(ctx, image, slot), W, H, lvl(s.down, 0), w0, h0, b->MaxColor, b->Threshold);
    // down pass l: down level l - 1 -> down level l; Lod = l - 1, so the pass that writes level 1 prefilters again (compute.glsl:41, Bloom.cs:85)
    for (int l = 1; l < levels; l++)
        hipLaunchKernelGGL((k_bloom_pass<0>), grid(dim(w0, l), dim(h0, l)), dim3(256), 0, ctx->stream, (const uint2*)lvl(s.down, l - 1), (const uint2*)nullptr, dim(w0, l - 1), dim(h0, l - 1), lvl(s.down, l), dim(w0, l), dim(h0, l), l == 1 ? 1 : 0, b->MaxColor, b->Threshold);
    // up passes: up level l from Upsample(level l + 1 of the up chain — of the DOWN chain in the first pass, Bloom.cs:98) + down level l + 1 (Lod = l + 1 for both samplers)
    for (int l = levels - 2; l >= 0; l--) {
        const uint2* a = l == levels - 2 ? lvl(s.down, l + 1) : lvl(s.up, l + 1);
        hipLaunchKernelGGL((k_bloom_pass<1>), grid(dim(w0, l), dim(h0, l)), dim3(256), 0, ctx->stream, a, (const uint2*)lvl(s.down, l + 1), dim(w0, l + 1), dim(h0, l + 1), lvl(s.up, l), dim(w0, l), dim(h0, l), 0, 0.0f, 0.0f);
    }
    hipLaunchKernelGGL(k_bloom_expand, dim3((unsigned)(((size_t)pw * ph + 255) / 256)), dim3(256), 0, ctx->stream, (const uint2*)lvl(s.up, 0), w0, h0, s.out.as<float4>(), pw, ph);
    HIPC(hipGetLastError());
    s.levels = levels; s.w0 = w0; s.h0 = h0; s.direct = direct; s.valid = true;
    return IDKPT_OK;
}
#define BLOOM_NONE ": the slot was not bloomed since the last resize (idkptBloom)"
static int32_t dev_GetBloomInfo(dev_ctx* ctx, int32_t slot, int32_t* levels, int32_t* w0, int32_t* h0)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    BloomSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.bloom, "idkptGetBloomInfo", slot, BLOOM_NONE, &s); if (rc) return rc; }
    if (levels) *levels = s->levels;
    if (w0) *w0 = s->w0;
    if (h0) *h0 = s->h0;
    return IDKPT_OK;
}
// a whole chain as it lies in memory (the levels one behind the other, level 0 first): *outBytes in front of the chain's guard
static int32_t dev_GetBloomChainDevicePtr(dev_ctx* ctx, int32_t slot, int32_t chain, void** outPtr, size_t* outBytes)
{
    if (!ctx || !outPtr) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(chain == 0 || chain == 1, "idkptGetBloomChainDevicePtr: chain must be 0 (down) or 1 (up)");
    BloomSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.bloom, "idkptGetBloomChainDevicePtr", slot, BLOOM_NONE, &s); if (rc) return rc; }
    const GuardedBuf& b = chain ? s->up : s->down;
    *outPtr = b.mem.p;
    if (outBytes) *outBytes = b.bytes;
    return IDKPT_OK;
}
static int32_t dev_GetBloomRoute(dev_ctx* ctx, int32_t slot, int32_t* route)
{
    if (!ctx || !route) return IDKPT_ERR_INVALID_ARGUMENT;
    BloomSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.bloom, "idkptGetBloomRoute", slot, BLOOM_NONE, &s); if (rc) return rc; }
    *route = s->direct ? IDKPT_BLOOM_ROUTE_DIRECT : IDKPT_BLOOM_ROUTE_TILED;
    return IDKPT_OK;
}
static int32_t dev_DownloadBloom(dev_ctx* ctx, int32_t slot, int32_t chain, int32_t level, void* dst, size_t bytes)
{
    if (!ctx || !dst) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(chain == 0 || chain == 1, "idkptDownloadBloom: chain must be 0 (down) or 1 (up)");
    BloomSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.bloom, "idkptDownloadBloom", slot, BLOOM_NONE, &s); if (rc) return rc; }
    REQUIRE(level >= 0 && level < s->levels - chain, "idkptDownloadBloom: level outside the chain (the down chain has `levels` levels, the up chain one fewer)");
    const size_t need = bloom_level_texels(s->w0, s->h0, level) * 8;
    REQUIRE(bytes == need, "idkptDownloadBloom: bytes must equal the level's width*height*8");
    return download_behind_queue(ctx, dst, (chain ? s->up : s->down).as<const char>() + bloom_level_offset(s->w0, s->h0, level) * 8, need);
}
static int32_t dev_GetBloomDevicePtr(dev_ctx* ctx, int32_t slot, void** outPtr, size_t* outBytes)
{
    if (!ctx || !outPtr) return IDKPT_ERR_INVALID_ARGUMENT;
    BloomSlot* s = nullptr;
    { int rc = slot_of(ctx, ctx->products.bloom, "idkptGetBloomDevicePtr", slot, BLOOM_NONE, &s); if (rc) return rc; }
    *outPtr = s->out.mem.p;
    if (outBytes) *outBytes = s->out.bytes;
    return IDKPT_OK;
}
