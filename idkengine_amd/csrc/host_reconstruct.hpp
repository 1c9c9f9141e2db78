// host_reconstruct.hpp — idkptReconstructHistory: the pixels of a ring slot's temporal image whose count is below FillBelow (the ones reprojection refused: occlusion
// edges, newly visible regions, the image border) are topped up with colour gathered from texels of the same surface that kept their history (kernel:
// kernels_reconstruct.hpp; the contract: include/idkpt.h, "history reconstruction").  Part of the single translation unit idkpt.hip (included there, behind
// host_reproject.hpp, whose slot records and scope it uses).  The kernel works IN PLACE (the argument: reconstruct_texel.hpp): no spare image, no swap, the temporal
// image stays where it is and a pointer from idkptGetTemporalDevicePtr stays valid.  Nothing but the temporal rgb is written: the counts, the temporal moments, the fast
// temporal image and the accumulation are as they were.  Queued samples are launched first, the call is stream-ordered and waits for nothing.
#pragma once

static int32_t dev_ReconstructHistory(dev_ctx* ctx, int32_t slot, const idkpt_reconstruct* r)
{
    if (!ctx || !r) return IDKPT_ERR_INVALID_ARGUMENT;
    auto positive = [](float v) { return reprojt::finite(v) && v > 0.0f; };
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptReconstructHistory: slot outside the frame ring (-1: the current slot)");
    REQUIRE(r->Radius >= 1 && r->Radius <= recont::MAX_RADIUS, "idkptReconstructHistory: Radius must be 1, 2 or 3");
    REQUIRE(r->Stride >= 1 && r->Stride <= recont::MAX_STRIDE, "idkptReconstructHistory: Stride must be 1..8");
    REQUIRE(positive(r->FillBelow), "idkptReconstructHistory: FillBelow must be finite and > 0");
    REQUIRE(positive(r->AlbedoSigma) && positive(r->NormalSigma), "idkptReconstructHistory: AlbedoSigma and NormalSigma must be finite and > 0");
    { int rc = denoise_scope(ctx, "idkptReconstructHistory"); if (rc) return rc; }
    if (!ctx->st.OutputAOVs) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptReconstructHistory: the current settings have OutputAOVs = 0: the albedo and normal images that guide the gather are not accumulated");
    TemporalSlot* t = nullptr;
    { int rc = temporal_slot_of(ctx, "idkptReconstructHistory", slot, GEOMETRY_IMAGE, &t); if (rc) return rc; }
    { int rc = temporal_slot_of(ctx, "idkptReconstructHistory", slot, TEMPORAL_IMAGE, &t); if (rc) return rc; }
    if (slot < 0) slot = ctx->curSlot;
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptReproject); the accumulation is not touched
    recont::Params p;
    p.W = ctx->W; p.H = ctx->H; p.stride = r->Stride; p.fillBelow = r->FillBelow;
    p.invA = denoiset::inv_sigma2(r->AlbedoSigma, 0); p.invN = denoiset::inv_sigma2(r->NormalSigma, 0);   // (as idkptDenoiseTemporal)
    const dim3 grid((unsigned)((p.W + denoisek::TILE - 1) / denoisek::TILE), (unsigned)((p.H + denoisek::TILE - 1) / denoisek::TILE));
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, t->temporal.as<float4>(), t->geom.as<const float4>(), (const float4*)image_ptr(ctx, IDKPT_IMAGE_ALBEDO, slot), (const float4*)image_ptr(ctx, IDKPT_IMAGE_NORMAL, slot), p); };
    if (r->Radius == 1) launch(k_reconstruct<1>);
    else if (r->Radius == 2) launch(k_reconstruct<2>);
    else launch(k_reconstruct<3>);
    HIPC(hipGetLastError());
    return IDKPT_OK;
}
