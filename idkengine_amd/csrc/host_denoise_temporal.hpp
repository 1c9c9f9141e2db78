// host_denoise_temporal.hpp — idkptDenoiseTemporal: the variance-guided filter on the TEMPORAL image of a ring slot, its variance made of the slot's temporal moments image
// with each pixel's own effective sample count (kernels: kernels_denoise_temporal.hpp for the first state, kernels_denoise_variance.hpp for the iterations; the contract:
// include/idkpt.h, "temporal moments").  Part of the single translation unit idkpt.hip (included there, behind host_denoise_variance.hpp, whose iteration and sigma
// check it uses on host_denoise.hpp's driver, and host_reproject.hpp, whose slot records it reads).  The fourth way to fill the DenoiseSlot (out, ping[2]): no buffer
// and no life-cycle rule is added, every call that reads a denoised image reads this one unchanged.  It ignores idkptSetDenoiseInput, needs neither the noise switch
// nor two samples, and reads neither Result nor the accumulated moments.  Queued samples are launched first, the call is stream-ordered and waits for nothing.
#pragma once

static int32_t dev_DenoiseTemporal(dev_ctx* ctx, int32_t slot, const idkpt_denoise_temporal* d)
{
    if (!ctx || !d) return IDKPT_ERR_INVALID_ARGUMENT;
    const bool below = noiset::finite(d->SpatialBelow) && d->SpatialBelow >= 2.0f;
    { int rc = denoise_check(ctx, "idkptDenoiseTemporal", slot, d->Iterations, d->DemodulateAlbedo, denoise_variance_sigmas(d->LumaSigma, d->VarianceEpsilon, d->AlbedoSigma, d->NormalSigma), below ? nullptr : ": SpatialBelow must be finite and >= 2"); if (rc) return rc; }
    TemporalSlot* t = nullptr;
    { int rc = temporal_slot_of(ctx, "idkptDenoiseTemporal", slot, TEMPORAL_IMAGE, &t); if (rc) return rc; }
    { int rc = temporal_slot_of(ctx, "idkptDenoiseTemporal", slot, TEMPORAL_MOMENTS_IMAGE, &t); if (rc) return rc; }
    if (slot < 0) slot = ctx->curSlot;
    DenoiseFill f;                                       // (the guides are the accumulated ones; the first state goes to ping[1], iteration i then writes ping[i & 1], the last one `out`)
    { int rc = denoise_begin(ctx, slot, d->Iterations, true, nullptr, &f); if (rc) return rc; }
    denoisetk::Params q;
    q.W = f.W; q.H = f.H; q.spatialBelow = d->SpatialBelow; q.demod = d->DemodulateAlbedo;
    q.invA = denoiset::inv_sigma2(d->AlbedoSigma, 0); q.invN = denoiset::inv_sigma2(d->NormalSigma, 0);
    hipLaunchKernelGGL(k_temporal_state, f.grid, dim3(256), 0, ctx->stream, t->temporal.as<const float4>(), t->moments.as<const float4>(), f.albedo, f.normal, f.s->ping[1].as<float4>(), q);
    denoisevk::Params p;
    p.W = f.W; p.H = f.H; p.n = 0u; p.demod = d->DemodulateAlbedo;
    p.ls2 = d->LumaSigma * d->LumaSigma; p.eps = d->VarianceEpsilon; p.invA = q.invA; p.invN = q.invN;
    return denoise_iterate(ctx, f, f.s->ping[1].as<const float4>(), [&](int, int spacing, int route, const float4* src, float4* dst, bool, bool last) {
        denoise_variance_iteration(ctx, f, p, spacing, route, src, nullptr, dst, false, last);   // (never the first_state of idkptDenoiseVariance: the pre-pass made the state)
    });
}
