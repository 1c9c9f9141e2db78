// host_denoise_temporal.hpp — idkptDenoiseTemporal: the variance-guided filter on the TEMPORAL image of a ring slot, its variance made of the slot's temporal moments image
// with each pixel's own effective sample count (kernels: kernels_denoise_temporal.hpp for the first state, kernels_denoise_variance.hpp for the iterations; the contract:
// include/idkpt.h, "temporal moments").  Part of the single translation unit idkpt.hip (included there, behind host_denoise_variance.hpp and host_reproject.hpp, whose
// scope checks and slot records it uses).  The fourth way to fill the DenoiseSlot (out, ping[2]): no buffer and no life-cycle rule is added, every call that reads a
// denoised image reads this one unchanged.  It ignores idkptSetDenoiseInput, needs neither the noise switch nor two samples, and reads neither Result nor the accumulated
// moments.  Queued samples are launched first, the call is stream-ordered and waits for nothing.
#pragma once

static int32_t dev_DenoiseTemporal(dev_ctx* ctx, int32_t slot, const idkpt_denoise_temporal* d)
{
    if (!ctx || !d) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptDenoiseTemporal: slot outside the frame ring (-1: the current slot)");
    REQUIRE(d->Iterations >= 1 && d->Iterations <= denoiset::MAX_ITERATIONS, "idkptDenoiseTemporal: Iterations must be 1..8");
    auto positive = [](float v) { return noiset::finite(v) && v > 0.0f; };
    REQUIRE(positive(d->LumaSigma) && positive(d->VarianceEpsilon) && positive(d->AlbedoSigma) && positive(d->NormalSigma), "idkptDenoiseTemporal: LumaSigma, VarianceEpsilon, AlbedoSigma and NormalSigma must be finite and > 0");
    REQUIRE(d->DemodulateAlbedo == 0 || d->DemodulateAlbedo == 1, "idkptDenoiseTemporal: DemodulateAlbedo must be 0 or 1");
    REQUIRE(noiset::finite(d->SpatialBelow) && d->SpatialBelow >= 2.0f, "idkptDenoiseTemporal: SpatialBelow must be finite and >= 2");
    { int rc = denoise_scope(ctx, "idkptDenoiseTemporal"); if (rc) return rc; }
    if (!ctx->st.OutputAOVs) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoiseTemporal: the current settings have OutputAOVs = 0: the albedo and normal images that guide the filter are not accumulated");
    TemporalSlot* t = nullptr;
    { int rc = temporal_slot_of(ctx, "idkptDenoiseTemporal", slot, TEMPORAL_IMAGE, &t); if (rc) return rc; }
    { int rc = temporal_slot_of(ctx, "idkptDenoiseTemporal", slot, TEMPORAL_MOMENTS_IMAGE, &t); if (rc) return rc; }
    if (slot < 0) slot = ctx->curSlot;
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptDenoise): the guides are the accumulated ones
    { int rc = check_overflow(ctx); if (rc) return rc; }   // (no wait: see idkptGetFrameDevicePtr)
    const int W = ctx->W, H = ctx->H, n = d->Iterations;
    const size_t bytes = (size_t)W * H * 16;
    DenoiseSlot& s = FrameProducts::slot(ctx->products.denoise, ctx->ringSize, slot);
    s.valid = false; s.iterations = 0;
    HIPC(s.out.ensure(ctx->stream, bytes));
    HIPC(s.ping[1].ensure(ctx->stream, bytes));          // the first state; iteration i then writes ping[i & 1], the last one `out`
    if (n >= 2) HIPC(s.ping[0].ensure(ctx->stream, bytes));
    const float4* albedo = image_ptr(ctx, IDKPT_IMAGE_ALBEDO, slot); const float4* normal = image_ptr(ctx, IDKPT_IMAGE_NORMAL, slot);
    const dim3 grid((unsigned)((W + denoisek::TILE - 1) / denoisek::TILE), (unsigned)((H + denoisek::TILE - 1) / denoisek::TILE));
    denoisetk::Params q;
    q.W = W; q.H = H; q.spatialBelow = d->SpatialBelow; q.demod = d->DemodulateAlbedo;
    q.invA = denoiset::inv_sigma2(d->AlbedoSigma, 0); q.invN = denoiset::inv_sigma2(d->NormalSigma, 0);
    hipLaunchKernelGGL(k_temporal_state, grid, dim3(256), 0, ctx->stream, t->temporal.as<const float4>(), t->moments.as<const float4>(), albedo, normal, s.ping[1].as<float4>(), q);
    denoisevk::Params p;
    p.W = W; p.H = H; p.n = 0u; p.demod = d->DemodulateAlbedo; p.first = 0;   // (never the first_state of idkptDenoiseVariance: the pre-pass made the state)
    p.ls2 = d->LumaSigma * d->LumaSigma; p.eps = d->VarianceEpsilon; p.invA = q.invA; p.invN = q.invN;
    const float4* src = s.ping[1].as<const float4>();
    for (int i = 0; i < n; i++) {
        float4* dst = (i == n - 1 ? s.out : s.ping[i & 1]).as<float4>();
        p.s = 1 << i; p.last = i == n - 1;
        s.route[i] = (uint8_t)denoise_route(p.s);
        if (s.route[i] == IDKPT_DENOISE_ROUTE_DIRECT) hipLaunchKernelGGL(k_denoise_var_direct, grid, dim3(256), 0, ctx->stream, src, albedo, normal, dst, p);
        else if (p.s == 1) hipLaunchKernelGGL((k_denoise_var_tile<1>), grid, dim3(256), 0, ctx->stream, src, (const float4*)nullptr, albedo, normal, dst, p);
        else if (p.s == 2) hipLaunchKernelGGL((k_denoise_var_tile<2>), grid, dim3(256), 0, ctx->stream, src, (const float4*)nullptr, albedo, normal, dst, p);
        else hipLaunchKernelGGL((k_denoise_var_tile<4>), grid, dim3(256), 0, ctx->stream, src, (const float4*)nullptr, albedo, normal, dst, p);
        src = dst;
    }
    HIPC(hipGetLastError());
    s.iterations = n; s.valid = true;
    return IDKPT_OK;
}
