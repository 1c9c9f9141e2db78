// host_rectify.hpp — idkptRectifyHistory: where the fast and the long history of a ring slot disagree by more than their noise explains, the temporal image and its sample
// count are pulled towards the fast temporal image (kernel: kernels_rectify.hpp; the contract: include/idkpt.h, "history rectification").  Part of the single translation
// unit idkpt.hip (included there, behind host_reproject.hpp, whose slot records and scope it uses; idkptReprojectFast and the fast image's readers live there, beside
// idkptReproject).  The kernel reads neighbours' temporal texels, so it writes the context's spare image (FrameProducts::rectifySpare) and the two buffers are swapped:
// the slot's temporal image is the written one from then on — in stream order, as every reader of it is — and the read one is the next call's spare.  Queued samples are
// launched first, the call is stream-ordered and waits for nothing.
#pragma once

static int32_t dev_RectifyHistory(dev_ctx* ctx, int32_t slot, const idkpt_rectify* r)
{
    if (!ctx || !r) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptRectifyHistory: slot outside the frame ring (-1: the current slot)");
    REQUIRE(r->Radius >= 1 && r->Radius <= rectt::MAX_RADIUS, "idkptRectifyHistory: Radius must be 1, 2 or 3");
    REQUIRE(reprojt::finite(r->ZLow) && r->ZLow > 0.0f, "idkptRectifyHistory: ZLow must be finite and > 0");
    REQUIRE(reprojt::finite(r->ZHigh) && r->ZHigh > r->ZLow, "idkptRectifyHistory: ZHigh must be finite and > ZLow");
    REQUIRE(reprojt::finite(r->Epsilon) && r->Epsilon > 0.0f, "idkptRectifyHistory: Epsilon must be finite and > 0");
    { int rc = denoise_scope(ctx, "idkptRectifyHistory"); if (rc) return rc; }
    TemporalSlot* t = nullptr;
    { int rc = temporal_slot_of(ctx, "idkptRectifyHistory", slot, GEOMETRY_IMAGE, &t); if (rc) return rc; }
    { int rc = temporal_slot_of(ctx, "idkptRectifyHistory", slot, TEMPORAL_IMAGE, &t); if (rc) return rc; }
    { int rc = temporal_slot_of(ctx, "idkptRectifyHistory", slot, FAST_TEMPORAL_IMAGE, &t); if (rc) return rc; }
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptReproject); the accumulation is not touched
    const int W = ctx->W, H = ctx->H;
    GuardedBuf& spare = ctx->products.rectifySpare;
    HIPC(spare.ensure(ctx->stream, (size_t)W * H * 16));
    rectt::Params p;
    p.W = W; p.H = H;
    p.eps2 = r->Epsilon * r->Epsilon; p.lo2 = r->ZLow * r->ZLow; p.span = r->ZHigh * r->ZHigh - p.lo2;
    const dim3 grid((unsigned)((W + denoisek::TILE - 1) / denoisek::TILE), (unsigned)((H + denoisek::TILE - 1) / denoisek::TILE));
    float4* const moments = t->momentsValid ? t->moments.as<float4>() : nullptr;   // its count follows the blended alpha (idkptDenoiseTemporal reads the two as one)
    with_flag(moments != nullptr, [&](auto MOMENTS) {
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, t->temporal.as<const float4>(), t->fast.as<const float4>(), t->geom.as<const float4>(), spare.as<float4>(), moments, p); };
        if (r->Radius == 1) launch(k_rectify<1, MOMENTS>);
        else if (r->Radius == 2) launch(k_rectify<2, MOMENTS>);
        else launch(k_rectify<3, MOMENTS>);
    });
    HIPC(hipGetLastError());
    std::swap(t->temporal, spare);                       // (same payload size: both were ensured for this frame size)
    return IDKPT_OK;
}
