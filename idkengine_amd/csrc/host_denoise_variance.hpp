// host_denoise_variance.hpp — idkptDenoiseVariance: the variance-guided filter that fills the denoised image of a ring slot from Result, Albedo, Normal and the luminance
// moments (kernels: kernels_denoise_variance.hpp; the contract: include/idkpt.h).  Part of the single translation unit idkpt.hip (included there, behind host_noise.hpp and
// host_denoise.hpp, whose driver (denoise_check / denoise_begin / denoise_iterate / denoise_ladder) and moments images it uses).  It fills the DenoiseSlot idkptDenoise and idkptUploadDenoised fill (out, ping[2]: the
// variance travels in the alpha of the two ping images) and adds no buffer and no life-cycle rule; every call that reads a denoised image reads this one unchanged.
// Queued samples are launched first, the call is stream-ordered and waits for nothing.  denoise_variance_iteration is the one place that launches the family's kernels.
#pragma once

// one iteration of the variance-guided filter, for idkptDenoiseVariance and idkptDenoiseTemporal: p holds what does not change between the iterations; `moments` is read
// by the first iteration when `first` (then the state is made in its staging loop) and may be nullptr otherwise
static void denoise_variance_iteration(dev_ctx* ctx, const DenoiseFill& f, denoisevk::Params p, int spacing, int route, const float4* src, const float4* moments, float4* dst, bool first, bool last)
{
    p.s = spacing; p.first = first; p.last = last;
    denoise_ladder(route, spacing,
        [&](auto S) { hipLaunchKernelGGL((k_denoise_var_tile<decltype(S)::value>), f.grid, dim3(256), 0, ctx->stream, src, moments, f.albedo, f.normal, dst, p); },
        [&] { hipLaunchKernelGGL(k_denoise_var_direct, f.grid, dim3(256), 0, ctx->stream, src, f.albedo, f.normal, dst, p); });
}
// the sigmas of the two: what denoise_check says (nullptr: nothing) unless all four are finite and > 0
static const char* denoise_variance_sigmas(float luma, float eps, float albedo, float normal)
{
    auto positive = [](float v) { return noiset::finite(v) && v > 0.0f; };
    return positive(luma) && positive(eps) && positive(albedo) && positive(normal) ? nullptr : ": LumaSigma, VarianceEpsilon, AlbedoSigma and NormalSigma must be finite and > 0";
}

static int32_t dev_DenoiseVariance(dev_ctx* ctx, int32_t slot, const idkpt_denoise_variance* d)
{
    if (!ctx || !d) return IDKPT_ERR_INVALID_ARGUMENT;
    { int rc = denoise_check(ctx, "idkptDenoiseVariance", slot, d->Iterations, d->DemodulateAlbedo, denoise_variance_sigmas(d->LumaSigma, d->VarianceEpsilon, d->AlbedoSigma, d->NormalSigma)); if (rc) return rc; }
    { int rc = noise_scope(ctx, "idkptDenoiseVariance"); if (rc) return rc; }
    if (ctx->denoiseInput == IDKPT_DENOISE_INPUT_TEMPORAL)   // (per-pixel sample counts and reprojected moments are idkptDenoiseTemporal's: host_denoise_temporal.hpp)
        return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoiseVariance: the denoise input is IDKPT_DENOISE_INPUT_TEMPORAL (idkptSetDenoiseInput): the moments are those of the accumulated image, not of the temporal one");
    if (slot < 0) slot = ctx->curSlot;
    const uint32_t samples = ctx->accum[slot];           // (queued samples included: they are launched below)
    if (samples < 2u) return fail(ctx, IDKPT_ERR_INVALID_OPERATION, "idkptDenoiseVariance: the slot has accumulated fewer than 2 samples: a variance needs two");
    DenoiseFill f;
    { int rc = denoise_begin(ctx, slot, d->Iterations, false, noise_moments_ensure, &f); if (rc) return rc; }
    denoisevk::Params p;
    p.W = f.W; p.H = f.H; p.n = samples; p.demod = d->DemodulateAlbedo;
    p.ls2 = d->LumaSigma * d->LumaSigma; p.eps = d->VarianceEpsilon; p.invA = denoiset::inv_sigma2(d->AlbedoSigma, 0); p.invN = denoiset::inv_sigma2(d->NormalSigma, 0);
    return denoise_iterate(ctx, f, image_ptr(ctx, IDKPT_IMAGE_RESULT, slot), [&](int, int spacing, int route, const float4* src, float4* dst, bool first, bool last) {
        denoise_variance_iteration(ctx, f, p, spacing, route, src, noise_moments_ptr(ctx, slot), dst, first, last);
    });
}
