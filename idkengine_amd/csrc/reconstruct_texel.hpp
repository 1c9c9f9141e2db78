// reconstruct_texel.hpp — the per-pixel arithmetic of idkptReconstructHistory (the contract of include/idkpt.h, "history reconstruction"): a pixel whose temporal count
// is below FillBelow gathers colour from the texels of the same surface at p + Stride * (dx, dy) that kept a count of at least FillBelow, weighted by the guide kernels
// of the filters and by their counts, and is topped up with it to at most FillBelow samples' worth.  Written once for the device (kernels_reconstruct.hpp) and for a host
// compiler (tests/c_driver/reconstruct_host.cpp builds this file with g++ under ASan/UBSan).  Depends on <math.h>, <stdint.h> and <string.h> only (through
// reproject_texel.hpp, whose V4, finite, bits_of and MISS_ID it uses, and denoise_texel.hpp, whose V3 and dist2).  No counterpart in the reference.
//
// Every operation is a binary32 + - * / in the written order (the library is compiled with -ffp-contract=off: nothing is fused; `/` is the IEEE division; fminf ignores
// a NaN operand), so tests/reconstruct_ref.py restates the same text in numpy and is compared bit for bit.  No value feeds an address: a NaN, an infinity or a
// difference that overflowed only drops its tap, or leaves the pixel as it is.
//
// IN PLACE: a written pixel has a count below FillBelow, a tap that contributes has a count of at least FillBelow, and the count is never written.  So no pixel's result
// depends on a texel another pixel writes: the result is that of the input image whatever the order in which the pixels run, and the caller may store it where it read.
#pragma once
#include <math.h>
#include <stdint.h>
#include "reproject_texel.hpp"
#include "denoise_texel.hpp"

namespace recont {

using reprojt::V4;
using reprojt::v4;
using reprojt::finite;
using reprojt::bits_of;
using denoiset::V3;

constexpr int MAX_RADIUS = 3;
constexpr int MAX_STRIDE = 8;

struct Params {
    int W, H, stride;
    float fillBelow;
    float invA, invN;                     // denoiset::inv_sigma2 of AlbedoSigma and NormalSigma at iteration 0: computed once per call on the host in binary32
};

struct Texel { V4 out; bool written; };   // written: out differs from nothing but the pixel's rgb; not written: the pixel keeps its 16 bytes

REPROJECT_HD bool finite4(V4 q) { return finite(q.x) && finite(q.y) && finite(q.z) && finite(q.w); }

// Pixel (x, y) of a W x H image.  fetch.history(qx, qy, &t, &id) returns the temporal texel and the bits of the geometry record's .w of an IN-IMAGE texel,
// fetch.guides(qx, qy, &a, &n) its accumulated albedo and normal; neither is called for a texel outside.  The guides are asked for only behind the tests on the history:
// of the pixel itself once it is known to be filled, of a tap once it is known to hold the same surface and a long enough history.  dy is the outer loop, dx the inner one.
template <int R, class Fetch>
REPROJECT_HD Texel reconstruct_texel(const Fetch& fetch, const Params& p, int x, int y)
{
    static_assert(R >= 1 && R <= MAX_RADIUS, "the taps span 3 x 3, 5 x 5 or 7 x 7 positions");
    Texel r; r.written = false;
    V4 tp; uint32_t id;
    fetch.history(x, y, &tp, &id);
    r.out = tp;
    const float c = tp.w;
    if (id == reprojt::MISS_ID || !finite4(tp) || !(c < p.fillBelow)) return r;
    V3 ap, np;
    fetch.guides(x, y, &ap, &np);
    float S = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int dy = -R; dy <= R; dy++) {
        const int qy = y + p.stride * dy;
        if (qy < 0 || qy >= p.H) continue;
        for (int dx = -R; dx <= R; dx++) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + p.stride * dx;
            if (qx < 0 || qx >= p.W) continue;
            V4 tq; uint32_t idq;
            fetch.history(qx, qy, &tq, &idq);
            if (idq != id || !finite4(tq) || !(tq.w >= p.fillBelow)) continue;
            V3 aq, nq;
            fetch.guides(qx, qy, &aq, &nq);
            const float w = 1.0f / ((1.0f + denoiset::dist2(aq, ap) * p.invA) * (1.0f + denoiset::dist2(nq, np) * p.invN));
            if (!(w > 0.0f)) continue;                // (false for a NaN weight and for the zero weight of an overflowed difference)
            const float k = w * tq.w;
            S = S + k;
            sx = sx + tq.x * k; sy = sy + tq.y * k; sz = sz + tq.z * k;
        }
    }
    if (!(S > 0.0f)) return r;
    const float b = fminf(S, p.fillBelow - c);
    const float den = c + b;
    const V4 o = v4((tp.x * c + (sx / S) * b) / den, (tp.y * c + (sy / S) * b) / den, (tp.z * c + (sz / S) * b) / den, c);
    if (!finite(o.x) || !finite(o.y) || !finite(o.z)) return r;
    r.out = o; r.written = true;
    return r;
}

}  // namespace recont
