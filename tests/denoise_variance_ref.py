"""The numpy restatement of idkptDenoiseVariance, written from the contract in include/idkpt.h ("variance-guided denoised output"), not from the C++: the a-trous filter
whose luminance range kernel follows the prefiltered variance of the pixel's mean luminance, every operation a binary32 + - * / in the header's order.  numpy's float32
array arithmetic rounds each operation correctly and fuses nothing, so the result is the contract's bit for bit; tests/test_denoise_variance_ref.py holds the host build of
csrc/denoise_variance_texel.hpp to it, tests/test_gpu_denoise_variance.py the device.

Two experiments of the non-finite rules (both (H, W) bool masks):
 `skip`     every tap AT a masked position is skipped, in the 25 taps AND in the 3 x 3 prefilter, as if that position were outside the image;
 `tapskip`  a masked position is skipped in the 25 taps of every OTHER pixel (its own tap on itself stays), the prefilter still reads its variance."""
import numpy as np

F = np.float32
K = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], F)
B = np.array([1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0], F)
EPS = F(1e-3)
DEFAULTS = dict(Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1)   # include/idkpt.h, profiles/denoise_variance.md
ROUTE_TILED, ROUTE_DIRECT = 0, 1


def route(iteration):
    """include/idkpt.h enum idkpt_denoise_route: spacing 1, 2, 4 staged in LDS, 8 and up fetched from memory"""
    return ROUTE_TILED if (1 << iteration) <= 4 else ROUTE_DIRECT


def inv_sigma2(sigma):
    with np.errstate(all="ignore"):
        s = F(sigma)
        return F(1.0) / F(s * s)


def floor_albedo(a):
    return np.fmax(a, EPS)                     # fmaxf: a NaN channel acts as eps


def lum(u):
    return (F(0.2126) * u[..., 0] + F(0.7152) * u[..., 1]) + F(0.0722) * u[..., 2]


def variance_of_mean(moments, N):
    """v0 (H, W): fmaxf(m2 - m1 * m1, 0) / (float)(N - 1); +Inf where a moment is not finite"""
    m1, m2 = np.asarray(moments, F)[..., 0], np.asarray(moments, F)[..., 1]
    with np.errstate(all="ignore"):
        v = np.fmax(m2 - m1 * m1, F(0.0)) / F(int(N) - 1)
    return np.where(np.isfinite(m1) & np.isfinite(m2), v, F(np.inf)).astype(F)


def first_state(result, albedo, moments, N, DemodulateAlbedo):
    """(c0 (H, W, 3), v0 (H, W)) as the first iteration reads them"""
    c = np.ascontiguousarray(np.asarray(result, F)[..., :3]); a = np.asarray(albedo, F)[..., :3]
    v = variance_of_mean(moments, N)
    with np.errstate(all="ignore"):
        if DemodulateAlbedo:
            fa = floor_albedo(a)
            c = (c / fa).astype(F)
            la = lum(fa)
            v = (v / (la * la)).astype(F)
    return c, v


def _dist2(u, P, Q):
    d = u[Q] - u[P]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _windows(H, W, s, dx, dy):
    y0, y1 = max(0, -s * dy), min(H, H - s * dy)
    x0, x1 = max(0, -s * dx), min(W, W - s * dx)
    if y0 >= y1 or x0 >= x1:
        return None                            # every such tap is outside the image: skipped
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))


def prefilter(v, skip=None):
    """g (H, W): the 3 x 3 binomial of v at spacing 1 over the taps that are inside and finite (NaN where there is none: only at pixels the filter leaves alone)"""
    H, W = v.shape
    fin = np.isfinite(v)
    if skip is not None:
        fin = fin & ~skip
    sumGV = np.zeros((H, W), F); sumG = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for ey in range(-1, 2):                # the outer loop
            for ex in range(-1, 2):            # the inner loop
                win = _windows(H, W, 1, ex, ey)
                if win is None:
                    continue
                P, Q = win
                gw = F(B[ex + 1] * B[ey + 1])
                sumGV[P] = np.where(fin[Q], sumGV[P] + gw * v[Q], sumGV[P])
                sumG[P] = np.where(fin[Q], sumG[P] + gw, sumG[P])
        return (sumGV / sumG).astype(F)


def iteration(c, v, a, n, s, ls2, eps, invA, invN, skip=None, tapskip=None):
    """one iteration with tap spacing s; c, a, n: (H, W, 3), v: (H, W) float32 -> (c, v)"""
    H, W = v.shape
    one = F(1.0)
    fin = np.isfinite(v)
    acc = np.zeros((H, W, 3), F); accV = np.zeros((H, W), F); accW = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        g = prefilter(v, skip)
        invL = one / (ls2 * g + eps)
        L = lum(c)
        for dy in range(-2, 3):                # the outer loop
            for dx in range(-2, 3):            # the inner loop
                win = _windows(H, W, s, dx, dy)
                if win is None:
                    continue
                P, Q = win
                h = F(K[dx + 2] * K[dy + 2])
                dl = L[Q] - L[P]
                den = ((one + (dl * dl) * invL[P]) * (one + _dist2(a, P, Q) * invA)) * (one + _dist2(n, P, Q) * invN)
                w = h / den
                ok = (w > 0) & fin[Q]          # w > 0: false for NaN and for 0
                if skip is not None:
                    ok = ok & ~skip[Q]
                if tapskip is not None and (dx, dy) != (0, 0):
                    ok = ok & ~tapskip[Q]
                acc[P] = np.where(ok[..., None], acc[P] + c[Q] * w[..., None], acc[P])
                accV[P] = np.where(ok, accV[P] + v[Q] * (w * w), accV[P])
                accW[P] = np.where(ok, accW[P] + w, accW[P])
        keep = (accW == 0) | ~fin               # a variance that is not finite, or no tap left: the pixel is unchanged
        cout = np.where(keep[..., None], c, acc / accW[..., None]).astype(F)
        vout = np.where(keep, v, accV / (accW * accW)).astype(F)
    return cout, vout


def filter_state(c, v, albedo, normal, Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, skip=None, tapskip=None):
    """the iterations alone, on a given state (c (H, W, 3), v (H, W)): what the contract carries from launch to launch -> (c, v)"""
    a = np.ascontiguousarray(np.asarray(albedo, F)[..., :3]); n = np.ascontiguousarray(np.asarray(normal, F)[..., :3])
    ls2 = F(F(LumaSigma) * F(LumaSigma)); eps = F(VarianceEpsilon)
    invA, invN = inv_sigma2(AlbedoSigma), inv_sigma2(NormalSigma)
    c = np.ascontiguousarray(c, F); v = np.ascontiguousarray(v, F)
    for i in range(int(Iterations)):
        c, v = iteration(c, v, a, n, 1 << i, ls2, eps, invA, invN, skip, tapskip)
    return c, v


def denoise_variance(result, albedo, normal, moments, N, Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1, skip=None, tapskip=None):
    """(H, W, 4) float32: rgb as the contract defines it, alpha 1.0.  result, albedo, normal, moments: (H, W, >= 3 / >= 2) float32 images as accumulated; N: the sample count"""
    c, v = first_state(result, albedo, moments, N, DemodulateAlbedo)
    c, v = filter_state(c, v, albedo, normal, Iterations, LumaSigma, VarianceEpsilon, AlbedoSigma, NormalSigma, skip, tapskip)
    with np.errstate(all="ignore"):
        if DemodulateAlbedo:
            c = (c * floor_albedo(np.asarray(albedo, F)[..., :3])).astype(F)
    out = np.ones(c.shape[:2] + (4,), F)
    out[..., :3] = c
    return out


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


# ---- the inputs both test files share (seeded; nothing here depends on the code under test)
SHAPES = [(1, 1), (5, 3), (16, 16), (17, 16), (16, 17), (37, 23), (70, 41)]          # (W, H): the shapes of the issue
SAMPLES = 2                                    # N of the shared cases: what the GPU tests render before they plant their images


def random_images(W, H, seed=0, N=SAMPLES):
    """Result, Albedo, Normal, Moments (H, W, 4) float32: smooth shading plus noise, albedo with channels at 0 and below eps in places, unit-ish normals in a few
    orientations; moments (m1, m2, 0, 1) with m1 near the luminance of Result and a per-pixel variance between 0 (m2 <= m1 * m1 in places: the clamp) and fireflies"""
    rng = np.random.default_rng(2000 * seed + 31 * W + H)
    y, x = np.mgrid[0:H, 0:W].astype(F)
    albedo = np.empty((H, W, 4), F); normal = np.empty((H, W, 4), F); result = np.empty((H, W, 4), F); moments = np.zeros((H, W, 4), F)
    block = ((x // 5).astype(int) + 2 * (y // 4).astype(int)) % 4
    palette = np.array([[0.8, 0.7, 0.6], [0.2, 0.5, 0.9], [0.0, 0.0005, 0.3], [0.95, 0.05, 0.0002]], F)      # channels at 0 and below eps
    normals = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [-0.70710677, 0.70710677, 0.0]], F)
    albedo[..., :3] = palette[block] + (rng.random((H, W, 3)) * 0.01).astype(F) * (palette[block] > 0.01)
    normal[..., :3] = normals[(block + (y // 7).astype(int)) % 4]
    shade = (0.4 + 0.3 * np.sin(x * F(0.37)) * np.cos(y * F(0.23))).astype(F)
    result[..., :3] = albedo[..., :3] * shade[..., None] * (0.5 + rng.random((H, W, 3))).astype(F) + (rng.random((H, W, 3)) * 0.02).astype(F)
    albedo[..., 3] = 1.0; normal[..., 3] = 1.0; result[..., 3] = 1.0
    m1 = lum(result[..., :3])
    spread = (F(10.0) ** (rng.random((H, W)) * 6.0 - 6.0).astype(F)) * (rng.random((H, W)) > 0.2)       # per-sample variance: 1e-6 .. 1, a fifth of the pixels 0
    m2 = (m1 * m1 + spread * F(N - 1) / F(N)).astype(F)
    m2 = np.where(rng.random((H, W)) < 0.1, m2 * F(0.5), m2).astype(F)                                     # m2 < m1 * m1: the clamp to 0
    moments[..., 0] = m1; moments[..., 1] = m2; moments[..., 3] = 1.0
    return result, albedo, normal, moments


NONFINITE = [("nan", F(np.nan)), ("+inf", F(np.inf)), ("-inf", F(-np.inf)), ("flt_max", np.finfo(F).max)]
PLANTS = [("colour", 0, 1), ("albedo", 1, 1), ("normal", 2, 1), ("m1", 3, 0), ("m2", 3, 1)]            # (name, image, channel)


def plant(images, which, value, pos, channel=1):
    """a copy of (result, albedo, normal, moments) with `value` in one channel of image `which` (0 .. 3) at pos = (x, y)"""
    out = [im.copy() for im in images]
    out[which][pos[1], pos[0], channel] = value
    return tuple(out)


def settings(Iterations, DemodulateAlbedo, LumaSigma=2.0, VarianceEpsilon=1e-3, AlbedoSigma=0.2, NormalSigma=0.5):
    return dict(Iterations=Iterations, LumaSigma=LumaSigma, VarianceEpsilon=VarianceEpsilon, AlbedoSigma=AlbedoSigma, NormalSigma=NormalSigma, DemodulateAlbedo=DemodulateAlbedo)


# (W, H, settings): the table of the issue.  1 x 1 with 1 and 8 iterations (every spacing beyond the image); 5 x 3 with 5 (from spacing 4 on every non-centre tap is
# outside); 16 x 16 with 1 and 2 (exactly one tile); 17 x 16 and 16 x 17 (one-pixel partial tiles); 37 x 23 with 4 and 8 (both routes, spacing larger than the image);
# 70 x 41 with 1, 3, 6 and the defaults (tile seams in both axes: first == last launch, every tiled spacing, both routes); DemodulateAlbedo 0 and 1
CASES = [
    (1, 1, settings(1, 1)), (1, 1, settings(8, 0)), (5, 3, settings(5, 1)), (5, 3, settings(5, 0)), (16, 16, settings(1, 1)), (16, 16, settings(1, 0)), (16, 16, settings(2, 0)), (16, 16, settings(2, 1)),
    (17, 16, settings(3, 1)), (16, 17, settings(3, 0)), (37, 23, settings(4, 1)), (37, 23, settings(4, 0)), (37, 23, settings(8, 0)), (37, 23, settings(8, 1)),
    (70, 41, settings(1, 0)), (70, 41, settings(1, 1)), (70, 41, settings(3, 1)), (70, 41, settings(6, 1)), (70, 41, settings(6, 0)), (70, 41, dict(DEFAULTS)),
]
PLANT_POS = (18, 11)                          # in the 37 x 23 image: interior, not on a tile seam's first column
PLANT_SETTINGS = [settings(4, 0), settings(4, 1)]      # spacing 1, 2, 4 (tiled) and 8 (direct)
