// host_reproject.hpp — idkptCaptureGeometry / idkptDownloadGeometry / idkptGetGeometryDevicePtr / idkptReproject / idkptDownloadTemporal / idkptGetTemporalDevicePtr /
// idkptUseTemporalAsDenoised / idkptSetDenoiseInput / idkptReprojectMoments / idkptDownloadTemporalMoments / idkptGetTemporalMomentsDevicePtr: the geometry image, the temporal
// image and the temporal moments image of a ring slot (kernels: kernels_reproject.hpp; the contract: include/idkpt.h, "temporal reprojection" and "temporal moments").  Part of the single translation unit idkpt.hip (included there, behind host_queries.hpp, whose closest-hit core traces the centre rays, and
// host_denoise.hpp, whose scope check and slot record it uses).
// Queued samples are launched first, nothing but the downloads waits for the GPU.  Frame products (host_context.hpp, "frame products": the life cycle of the buffers): a
// TemporalSlot per ring slot, all images RGBA32F of the render size; the ray and hit scratch of a capture belongs to the context and is sized for one frame.
// idkptCaptureMotion / idkptDownloadMotion / idkptGetMotionDevicePtr ("motion-aware capture"): the slot's fourth image, the previous world position of what each pixel
// sees; a slot that holds one is reprojected through it.  The previous vertex positions it reads (dev_ctx::motionPrev) are kept by host_scene.hpp.
// idkptReprojectFast / idkptDownloadFastTemporal / idkptGetFastTemporalDevicePtr ("history rectification"): the slot's fifth image, a second temporal image with a short
// cap, made by idkptReproject's body on another image pair; host_rectify.hpp compares the two.
// One device, the whole frame (the scope of idkptDenoise): a pixel's history may lie in any row.
#pragma once

// idkptCaptureGeometry (motion = false) and idkptCaptureMotion (motion = true): the centre rays of the current camera, their closest hits, and the records made of them —
// the geometry image alone (which drops the slot's motion image), or the geometry image and the motion image in one pass over the hits
static int32_t capture_records(dev_ctx* ctx, const std::string& who, int32_t slot, bool motion)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, who + ": slot outside the frame ring (-1: the current slot)");
    { int rc = denoise_scope(ctx, who.c_str()); if (rc) return rc; }
    if (!ctx->haveScene) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, who + ": no scene uploaded");
    if (slot < 0) slot = ctx->curSlot;
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptDenoise); the accumulation is not touched
    const int W = ctx->W, H = ctx->H;
    const size_t N = (size_t)W * ctx->rows;
    REQUIRE(N < (1ull << 31), who + ": too many pixels for one ray query");
    // Scene versions: the records are made of the CURRENT state (make_dscene's and vb_cur's slots), by kernels launched now.  A later update either finds the current slot
    // unpinned and writes it in place, behind these kernels on the stream, or moves on to another slot (ver_writable); motionPrev has one state and only stream-ordered writers.
    if (motion && !ctx->motionPrevOn) { int rc = motion_prev_reset(ctx); if (rc) return rc; }
    HIPC(ctx->geomRays.ensure(N * sizeof(idkpt_ray))); HIPC(ctx->geomHits.ensure(N * sizeof(idkpt_hit)));
    TemporalSlot& s = FrameProducts::slot(ctx->products.temporal, ctx->ringSize, slot);
    HIPC(s.geom.ensure(ctx->stream, N * 16));
    if (motion) HIPC(s.motion.ensure(ctx->stream, N * 16));
    reprojk::Camera cam;
    memcpy(cam.invProj, ctx->invProj, sizeof(cam.invProj)); memcpy(cam.invView, ctx->invView, sizeof(cam.invView));   // the camera current at the call
    const dim3 grid((unsigned)((N + 255) / 256));
    hipLaunchKernelGGL(k_geom_rays, grid, dim3(256), 0, ctx->stream, cam, W, H, (uint32_t)N, ctx->geomRays.as<idkpt_ray>());
    HIPC(hipGetLastError());
    { int rc = dev_TraceRaysDevice(ctx, ctx->geomRays.as<idkpt_ray>(), N, 0u, ctx->geomHits.as<idkpt_hit>()); if (rc) return rc; }   // closest hit, no lights: the core idkptTraceRaysDevice is held to the oracle with
    s.geomValid = false; s.motionValid = false;          // (a refused trace launched nothing: the previous records stay)
    if (motion)
        hipLaunchKernelGGL(k_geom_motion_pack, grid, dim3(256), 0, ctx->stream, (const idkpt_ray*)ctx->geomRays.as<idkpt_ray>(), (const idkpt_hit*)ctx->geomHits.as<idkpt_hit>(), (uint32_t)N,
                           (const uint4*)ctx->tris.as<uint4>(), (uint32_t)ctx->triCount, (const float*)ctx->motionPrev.as<float>(), (uint32_t)ctx->vertexCount,
                           (const float4*)vb_cur<float4>(ctx, VB_XFORMS), (uint32_t)ctx->xformCount, s.geom.as<float4>(), s.motion.as<float4>());
    else
        hipLaunchKernelGGL(k_geom_pack, grid, dim3(256), 0, ctx->stream, (const idkpt_ray*)ctx->geomRays.as<idkpt_ray>(), (const idkpt_hit*)ctx->geomHits.as<idkpt_hit>(), (uint32_t)N, s.geom.as<float4>());
    HIPC(hipGetLastError());
    s.geomValid = true; s.motionValid = motion;
    return IDKPT_OK;
}
static int32_t dev_CaptureGeometry(dev_ctx* ctx, int32_t slot) { return capture_records(ctx, "idkptCaptureGeometry", slot, false); }
static int32_t dev_CaptureMotion(dev_ctx* ctx, int32_t slot) { return capture_records(ctx, "idkptCaptureMotion", slot, true); }

// the record of ring slot `slot` (-1: the current one) for the calls that read one of its five images
enum TemporalImage { TEMPORAL_IMAGE = 0, GEOMETRY_IMAGE = 1, TEMPORAL_MOMENTS_IMAGE = 2, MOTION_IMAGE = 3, FAST_TEMPORAL_IMAGE = 4 };
static bool temporal_holds(const TemporalSlot& s, TemporalImage which) { return which == GEOMETRY_IMAGE ? s.geomValid : which == TEMPORAL_IMAGE ? s.temporalValid : which == MOTION_IMAGE ? s.motionValid : which == FAST_TEMPORAL_IMAGE ? s.fastValid : s.momentsValid; }
static const GuardedBuf& temporal_buf(const TemporalSlot& s, TemporalImage which) { return which == GEOMETRY_IMAGE ? s.geom : which == TEMPORAL_IMAGE ? s.temporal : which == MOTION_IMAGE ? s.motion : which == FAST_TEMPORAL_IMAGE ? s.fast : s.moments; }
static int32_t temporal_slot_of(dev_ctx* ctx, const char* who, int32_t slot, TemporalImage which, TemporalSlot** out)
{
    REQUIRE(slot >= -1 && slot < ctx->ringSize, std::string(who) + ": slot outside the frame ring (-1: the current slot)");
    if (slot < 0) slot = ctx->curSlot;
    std::vector<TemporalSlot>& v = ctx->products.temporal;
    if ((size_t)slot >= v.size() || !temporal_holds(v[slot], which))
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, std::string(who) + (which == GEOMETRY_IMAGE ? ": the slot holds no geometry image since the last resize (idkptCaptureGeometry)" : which == TEMPORAL_IMAGE ? ": the slot holds no temporal image since the last resize (idkptReproject)" : which == MOTION_IMAGE ? ": the slot holds no motion image (idkptCaptureMotion; idkptCaptureGeometry and every resize drop it)" : which == FAST_TEMPORAL_IMAGE ? ": the slot holds no fast temporal image since the last resize (idkptReprojectFast)" : ": the slot holds no temporal moments image since the last resize (idkptReprojectMoments)"));
    *out = &v[slot];
    return IDKPT_OK;
}
static int32_t temporal_download(dev_ctx* ctx, const char* who, int32_t slot, TemporalImage which, float* rgba, size_t bytes)
{
    if (!ctx || !rgba) return IDKPT_ERR_INVALID_ARGUMENT;
    TemporalSlot* s = nullptr;
    { int rc = temporal_slot_of(ctx, who, slot, which, &s); if (rc) return rc; }
    const GuardedBuf& b = temporal_buf(*s, which);
    REQUIRE(bytes == b.bytes, std::string(who) + ": bytes must equal height*width*16");
    return download_behind_queue(ctx, rgba, b.mem.p, bytes);
}
static int32_t temporal_device_ptr(dev_ctx* ctx, const char* who, int32_t slot, TemporalImage which, void** outPtr, size_t* outBytes)
{
    if (!ctx || !outPtr) return IDKPT_ERR_INVALID_ARGUMENT;
    TemporalSlot* s = nullptr;
    { int rc = temporal_slot_of(ctx, who, slot, which, &s); if (rc) return rc; }
    const GuardedBuf& b = temporal_buf(*s, which);
    *outPtr = b.mem.p;
    if (outBytes) *outBytes = b.bytes;
    return IDKPT_OK;
}
static int32_t dev_DownloadGeometry(dev_ctx* ctx, int32_t slot, float* rgba, size_t bytes) { return temporal_download(ctx, "idkptDownloadGeometry", slot, GEOMETRY_IMAGE, rgba, bytes); }
static int32_t dev_GetGeometryDevicePtr(dev_ctx* ctx, int32_t slot, void** outPtr, size_t* outBytes) { return temporal_device_ptr(ctx, "idkptGetGeometryDevicePtr", slot, GEOMETRY_IMAGE, outPtr, outBytes); }
static int32_t dev_DownloadTemporal(dev_ctx* ctx, int32_t slot, float* rgba, size_t bytes) { return temporal_download(ctx, "idkptDownloadTemporal", slot, TEMPORAL_IMAGE, rgba, bytes); }
static int32_t dev_GetTemporalDevicePtr(dev_ctx* ctx, int32_t slot, void** outPtr, size_t* outBytes) { return temporal_device_ptr(ctx, "idkptGetTemporalDevicePtr", slot, TEMPORAL_IMAGE, outPtr, outBytes); }
static int32_t dev_DownloadTemporalMoments(dev_ctx* ctx, int32_t slot, float* rgba, size_t bytes) { return temporal_download(ctx, "idkptDownloadTemporalMoments", slot, TEMPORAL_MOMENTS_IMAGE, rgba, bytes); }
static int32_t dev_GetTemporalMomentsDevicePtr(dev_ctx* ctx, int32_t slot, void** outPtr, size_t* outBytes) { return temporal_device_ptr(ctx, "idkptGetTemporalMomentsDevicePtr", slot, TEMPORAL_MOMENTS_IMAGE, outPtr, outBytes); }
static int32_t dev_DownloadMotion(dev_ctx* ctx, int32_t slot, float* rgba, size_t bytes) { return temporal_download(ctx, "idkptDownloadMotion", slot, MOTION_IMAGE, rgba, bytes); }
static int32_t dev_GetMotionDevicePtr(dev_ctx* ctx, int32_t slot, void** outPtr, size_t* outBytes) { return temporal_device_ptr(ctx, "idkptGetMotionDevicePtr", slot, MOTION_IMAGE, outPtr, outBytes); }
static int32_t dev_DownloadFastTemporal(dev_ctx* ctx, int32_t slot, float* rgba, size_t bytes) { return temporal_download(ctx, "idkptDownloadFastTemporal", slot, FAST_TEMPORAL_IMAGE, rgba, bytes); }
static int32_t dev_GetFastTemporalDevicePtr(dev_ctx* ctx, int32_t slot, void** outPtr, size_t* outBytes) { return temporal_device_ptr(ctx, "idkptGetFastTemporalDevicePtr", slot, FAST_TEMPORAL_IMAGE, outPtr, outBytes); }

// idkptReproject (which = TEMPORAL_IMAGE) and idkptReprojectFast (which = FAST_TEMPORAL_IMAGE): one body on the image pair (the history slot's image, the slot's image);
// the two calls differ in the pair and in what the messages call it
static int32_t reproject_image(dev_ctx* ctx, const std::string& who, TemporalImage which, int32_t slot, int32_t historySlot, const idkpt_reproject* r)
{
    if (!ctx || !r) return IDKPT_ERR_INVALID_ARGUMENT;
    const bool fast = which == FAST_TEMPORAL_IMAGE;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, who + ": slot outside the frame ring (-1: the current slot)");
    REQUIRE(historySlot == IDKPT_NO_HISTORY || (historySlot >= 0 && historySlot < ctx->ringSize), who + ": historySlot must be IDKPT_NO_HISTORY or a slot of the frame ring");
    REQUIRE(reprojt::finite(r->PositionTolerance) && r->PositionTolerance > 0.0f, who + ": PositionTolerance must be finite and > 0");
    REQUIRE(reprojt::finite(r->MaxHistory) && r->MaxHistory >= 1.0f, who + ": MaxHistory must be finite and >= 1");
    if (slot < 0) slot = ctx->curSlot;
    REQUIRE(slot != historySlot, who + ": slot and historySlot must differ (a frame is no history of itself)");
    { int rc = denoise_scope(ctx, who.c_str()); if (rc) return rc; }
    std::vector<TemporalSlot>& v = ctx->products.temporal;
    auto holds = [&](int q, TemporalImage im) { return (size_t)q < v.size() && temporal_holds(v[q], im); };
    if (!holds(slot, GEOMETRY_IMAGE)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, who + ": the slot holds no geometry image since the last resize (idkptCaptureGeometry)");
    const bool start = historySlot == IDKPT_NO_HISTORY;
    if (!start && !holds(historySlot, GEOMETRY_IMAGE)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, who + ": the history slot holds no geometry image since the last resize (idkptCaptureGeometry)");
    if (!start && !holds(historySlot, which)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, who + (fast ? ": the history slot holds no fast temporal image since the last resize (idkptReprojectFast)" : ": the history slot holds no temporal image since the last resize (idkptReproject)"));
    const uint32_t n = ctx->accum[slot];                 // (queued samples included: they are launched below)
    if (n == 0u) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, who + ": the slot has accumulated no sample");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptDenoise)
    { int rc = check_overflow(ctx); if (rc) return rc; }   // (no wait: see idkptGetFrameDevicePtr)
    const int W = ctx->W, H = ctx->H;
    TemporalSlot& s = v[slot];
    GuardedBuf& dst = fast ? s.fast : s.temporal;
    bool& dstValid = fast ? s.fastValid : s.temporalValid;
    dstValid = false;
    HIPC(dst.ensure(ctx->stream, (size_t)W * H * 16));
    reprojt::Params p;
    p.W = W; p.H = H;
    memcpy(p.M, r->PrevProjView, sizeof(p.M)); memcpy(p.prevPos, r->PrevViewPos, sizeof(p.prevPos));
    p.tol2 = r->PositionTolerance * r->PositionTolerance; p.maxHistory = r->MaxHistory; p.n = (float)n;
    const dim3 grid((unsigned)((W + reprojk::TILE - 1) / reprojk::TILE), (unsigned)((H + reprojk::TILE - 1) / reprojk::TILE));
    const float4* hg = start ? nullptr : v[historySlot].geom.as<const float4>();
    const float4* hc = start ? nullptr : temporal_buf(v[historySlot], which).as<const float4>();
    if (!start && s.motionValid)                         // the slot's surfaces are looked up where they stood in the history frame (idkptCaptureMotion)
        hipLaunchKernelGGL(k_reproject_motion<false>, grid, dim3(256), 0, ctx->stream, (const float4*)image_ptr(ctx, IDKPT_IMAGE_RESULT, slot), s.geom.as<const float4>(), s.motion.as<const float4>(), hg, hc, dst.as<float4>(), p);
    else
        hipLaunchKernelGGL(k_reproject, grid, dim3(256), 0, ctx->stream, (const float4*)image_ptr(ctx, IDKPT_IMAGE_RESULT, slot), s.geom.as<const float4>(), hg, hc, dst.as<float4>(), p);
    HIPC(hipGetLastError());
    dstValid = true;
    return IDKPT_OK;
}
static int32_t dev_Reproject(dev_ctx* ctx, int32_t slot, int32_t historySlot, const idkpt_reproject* r) { return reproject_image(ctx, "idkptReproject", TEMPORAL_IMAGE, slot, historySlot, r); }
static int32_t dev_ReprojectFast(dev_ctx* ctx, int32_t slot, int32_t historySlot, const idkpt_reproject* r) { return reproject_image(ctx, "idkptReprojectFast", FAST_TEMPORAL_IMAGE, slot, historySlot, r); }

// the luminance moments of the slot through the same taps: (m1, m2) of the moments image FinalDraw keeps (host_noise.hpp) blended with the history slot's temporal moments
// image; independent of idkptReproject (neither reads what the other writes)
static int32_t dev_ReprojectMoments(dev_ctx* ctx, int32_t slot, int32_t historySlot, const idkpt_reproject* r)
{
    if (!ctx || !r) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptReprojectMoments: slot outside the frame ring (-1: the current slot)");
    REQUIRE(historySlot == IDKPT_NO_HISTORY || (historySlot >= 0 && historySlot < ctx->ringSize), "idkptReprojectMoments: historySlot must be IDKPT_NO_HISTORY or a slot of the frame ring");
    REQUIRE(reprojt::finite(r->PositionTolerance) && r->PositionTolerance > 0.0f, "idkptReprojectMoments: PositionTolerance must be finite and > 0");
    REQUIRE(reprojt::finite(r->MaxHistory) && r->MaxHistory >= 1.0f, "idkptReprojectMoments: MaxHistory must be finite and >= 1");
    if (slot < 0) slot = ctx->curSlot;
    REQUIRE(slot != historySlot, "idkptReprojectMoments: slot and historySlot must differ (a frame is no history of itself)");
    { int rc = denoise_scope(ctx, "idkptReprojectMoments"); if (rc) return rc; }
    { int rc = noise_scope(ctx, "idkptReprojectMoments"); if (rc) return rc; }
    std::vector<TemporalSlot>& v = ctx->products.temporal;
    auto holds = [&](int q, TemporalImage which) { return (size_t)q < v.size() && temporal_holds(v[q], which); };
    if (!holds(slot, GEOMETRY_IMAGE)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptReprojectMoments: the slot holds no geometry image since the last resize (idkptCaptureGeometry)");
    const bool start = historySlot == IDKPT_NO_HISTORY;
    if (!start && !holds(historySlot, GEOMETRY_IMAGE)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptReprojectMoments: the history slot holds no geometry image since the last resize (idkptCaptureGeometry)");
    if (!start && !holds(historySlot, TEMPORAL_MOMENTS_IMAGE)) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptReprojectMoments: the history slot holds no temporal moments image since the last resize (idkptReprojectMoments)");
    const uint32_t n = ctx->accum[slot];                 // (queued samples included: they are launched below)
    if (n == 0u) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptReprojectMoments: the slot has accumulated no sample");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptReproject)
    { int rc = check_overflow(ctx); if (rc) return rc; }   // (no wait: see idkptGetFrameDevicePtr)
    { int rc = noise_moments_ensure(ctx); if (rc) return rc; }
    const int W = ctx->W, H = ctx->H;
    TemporalSlot& s = v[slot];
    s.momentsValid = false;
    HIPC(s.moments.ensure(ctx->stream, (size_t)W * H * 16));
    reprojt::Params p;
    p.W = W; p.H = H;
    memcpy(p.M, r->PrevProjView, sizeof(p.M)); memcpy(p.prevPos, r->PrevViewPos, sizeof(p.prevPos));
    p.tol2 = r->PositionTolerance * r->PositionTolerance; p.maxHistory = r->MaxHistory; p.n = (float)n;
    const dim3 grid((unsigned)((W + reprojk::TILE - 1) / reprojk::TILE), (unsigned)((H + reprojk::TILE - 1) / reprojk::TILE));
    const float4* hg = start ? nullptr : v[historySlot].geom.as<const float4>();
    const float4* hm = start ? nullptr : v[historySlot].moments.as<const float4>();
    if (!start && s.motionValid)                         // (as idkptReproject: the same lookup record, so the count stays the temporal alpha)
        hipLaunchKernelGGL(k_reproject_motion<true>, grid, dim3(256), 0, ctx->stream, (const float4*)noise_moments_ptr(ctx, slot), s.geom.as<const float4>(), s.motion.as<const float4>(), hg, hm, s.moments.as<float4>(), p);
    else
        hipLaunchKernelGGL(k_reproject_moments, grid, dim3(256), 0, ctx->stream, (const float4*)noise_moments_ptr(ctx, slot), s.geom.as<const float4>(), hg, hm, s.moments.as<float4>(), p);
    HIPC(hipGetLastError());
    s.momentsValid = true;
    return IDKPT_OK;
}

// the device-side sibling of idkptUploadDenoised: the slot's temporal rgb, alpha 1.0, becomes its denoised image
static int32_t dev_UseTemporalAsDenoised(dev_ctx* ctx, int32_t slot)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptUseTemporalAsDenoised: slot outside the frame ring (-1: the current slot)");
    { int rc = denoise_scope(ctx, "idkptUseTemporalAsDenoised"); if (rc) return rc; }
    TemporalSlot* t = nullptr;
    { int rc = temporal_slot_of(ctx, "idkptUseTemporalAsDenoised", slot, TEMPORAL_IMAGE, &t); if (rc) return rc; }
    if (slot < 0) slot = ctx->curSlot;
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();
    const size_t N = (size_t)ctx->W * ctx->H;
    DenoiseSlot& s = denoise_slot_invalidated(ctx, slot);
    HIPC(s.out.ensure(ctx->stream, N * 16));
    hipLaunchKernelGGL(k_temporal_to_denoised, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, t->temporal.as<const float4>(), (uint32_t)N, s.out.as<float4>());
    HIPC(hipGetLastError());
    s.valid = true;
    return IDKPT_OK;
}

static int32_t dev_SetDenoiseInput(dev_ctx* ctx, int32_t input)
{
    if (!ctx) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(input == IDKPT_DENOISE_INPUT_ACCUMULATED || input == IDKPT_DENOISE_INPUT_TEMPORAL, "idkptSetDenoiseInput: input must be IDKPT_DENOISE_INPUT_ACCUMULATED or IDKPT_DENOISE_INPUT_TEMPORAL");
    if (input == IDKPT_DENOISE_INPUT_TEMPORAL && !owns_whole_frame(ctx))
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptSetDenoiseInput: the temporal image needs the whole frame on one device; this context holds a shard of the rows or is a member of a multi-device context");
    ctx->denoiseInput = input;
    return IDKPT_OK;
}
static int32_t dev_GetDenoiseInput(dev_ctx* ctx, int32_t* out) { if (!ctx || !out) return IDKPT_ERR_INVALID_ARGUMENT; *out = ctx->denoiseInput; return IDKPT_OK; }
