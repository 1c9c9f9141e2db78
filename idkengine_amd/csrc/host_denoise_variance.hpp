// host_denoise_variance.hpp — idkptDenoiseVariance: the variance-guided filter that fills the denoised image of a ring slot from Result, Albedo, Normal and the luminance
// moments (kernels: kernels_denoise_variance.hpp; the contract: include/idkpt.h).  Part of the single translation unit idkpt.hip (included there, behind host_noise.hpp and
// host_denoise.hpp, whose scope checks, slot record and moments images it uses).  It fills the DenoiseSlot idkptDenoise and idkptUploadDenoised fill (out, ping[2]: the
// variance travels in the alpha of the two ping images) and adds no buffer and no life-cycle rule; every call that reads a denoised image reads this one unchanged.
// Queued samples are launched first, the call is stream-ordered and waits for nothing.
#pragma once

static int32_t dev_DenoiseVariance(dev_ctx* ctx, int32_t slot, const idkpt_denoise_variance* d)
{
    if (!ctx || !d) return IDKPT_ERR_INVALID_ARGUMENT;
    REQUIRE(slot >= -1 && slot < ctx->ringSize, "idkptDenoiseVariance: slot outside the frame ring (-1: the current slot)");
    REQUIRE(d->Iterations >= 1 && d->Iterations <= denoiset::MAX_ITERATIONS, "idkptDenoiseVariance: Iterations must be 1..8");
    auto positive = [](float v) { return noiset::finite(v) && v > 0.0f; };
    REQUIRE(positive(d->LumaSigma) && positive(d->VarianceEpsilon) && positive(d->AlbedoSigma) && positive(d->NormalSigma), "idkptDenoiseVariance: LumaSigma, VarianceEpsilon, AlbedoSigma and NormalSigma must be finite and > 0");
    REQUIRE(d->DemodulateAlbedo == 0 || d->DemodulateAlbedo == 1, "idkptDenoiseVariance: DemodulateAlbedo must be 0 or 1");
    { int rc = denoise_scope(ctx, "idkptDenoiseVariance"); if (rc) return rc; }
    if (!ctx->st.OutputAOVs) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoiseVariance: the current settings have OutputAOVs = 0: the albedo and normal images that guide the filter are not accumulated");
    { int rc = noise_scope(ctx, "idkptDenoiseVariance"); if (rc) return rc; }
    if (ctx->denoiseInput == IDKPT_DENOISE_INPUT_TEMPORAL)   // (per-pixel sample counts and reprojected moments are idkptDenoiseTemporal's: host_denoise_temporal.hpp)
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoiseVariance: the denoise input is IDKPT_DENOISE_INPUT_TEMPORAL (idkptSetDenoiseInput): the moments are those of the accumulated image, not of the temporal one");
    if (slot < 0) slot = ctx->curSlot;
    const uint32_t samples = ctx->accum[slot];           // (queued samples included: they are launched below)
    if (samples < 2u) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoiseVariance: the slot has accumulated fewer than 2 samples: a variance needs two");
    HIPC(hipSetDevice(ctx->device));
    FLUSH_KEEP();                                        // stream-ordered behind what was queued (as idkptDenoise)
    { int rc = check_overflow(ctx); if (rc) return rc; }   // (no wait: see idkptGetFrameDevicePtr)
    { int rc = noise_moments_ensure(ctx); if (rc) return rc; }
    const int W = ctx->W, H = ctx->H, n = d->Iterations;
    const size_t bytes = (size_t)W * H * 16;
    DenoiseSlot& s = FrameProducts::slot(ctx->products.denoise, ctx->ringSize, slot);
    s.valid = false; s.iterations = 0;
    HIPC(s.out.ensure(ctx->stream, bytes));
    for (int k = 0; k < 2 && k < n - 1; k++) HIPC(s.ping[k].ensure(ctx->stream, bytes));
    const float4* albedo = image_ptr(ctx, IDKPT_IMAGE_ALBEDO, slot); const float4* normal = image_ptr(ctx, IDKPT_IMAGE_NORMAL, slot);
    const float4* moments = noise_moments_ptr(ctx, slot);
    const dim3 grid((unsigned)((W + denoisek::TILE - 1) / denoisek::TILE), (unsigned)((H + denoisek::TILE - 1) / denoisek::TILE));
    denoisevk::Params p;
    p.W = W; p.H = H; p.n = samples; p.demod = d->DemodulateAlbedo;
    p.ls2 = d->LumaSigma * d->LumaSigma; p.eps = d->VarianceEpsilon; p.invA = denoiset::inv_sigma2(d->AlbedoSigma, 0); p.invN = denoiset::inv_sigma2(d->NormalSigma, 0);
    const float4* src = image_ptr(ctx, IDKPT_IMAGE_RESULT, slot);
    for (int i = 0; i < n; i++) {
        float4* dst = (i == n - 1 ? s.out : s.ping[i & 1]).as<float4>();
        p.s = 1 << i; p.first = i == 0; p.last = i == n - 1;
        s.route[i] = (uint8_t)denoise_route(p.s);
        if (s.route[i] == IDKPT_DENOISE_ROUTE_DIRECT) hipLaunchKernelGGL(k_denoise_var_direct, grid, dim3(256), 0, ctx->stream, src, albedo, normal, dst, p);
        else if (p.s == 1) hipLaunchKernelGGL((k_denoise_var_tile<1>), grid, dim3(256), 0, ctx->stream, src, moments, albedo, normal, dst, p);
        else if (p.s == 2) hipLaunchKernelGGL((k_denoise_var_tile<2>), grid, dim3(256), 0, ctx->stream, src, moments, albedo, normal, dst, p);
        else hipLaunchKernelGGL((k_denoise_var_tile<4>), grid, dim3(256), 0, ctx->stream, src, moments, albedo, normal, dst, p);
        src = dst;
    }
    HIPC(hipGetLastError());
    s.iterations = n; s.valid = true;
    return IDKPT_OK;
}
