"""The numpy restatement of idkptDenoise, written from the contract in include/idkpt.h ("denoised output"), not from the C++: the edge-avoiding a-trous filter with rational
range kernels, every operation a binary32 + - * / in the header's order.  numpy's float32 array arithmetic rounds each operation correctly and fuses nothing, so the result
is the contract's bit for bit; tests/test_denoise_ref.py holds the host build of csrc/denoise_texel.hpp to it, tests/test_gpu_denoise.py the device.

`skip` (an (H, W) bool mask) is the experiment of the non-finite rule: every tap AT a masked position is skipped, as if that position were outside the image."""
import numpy as np

F = np.float32
K = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], F)
EPS = F(1e-3)
DEFAULTS = dict(Iterations=5, ColorSigma=8.0, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1)   # include/idkpt.h, profiles/denoise.md
ROUTE_TILED, ROUTE_DIRECT = 0, 1


def route(iteration):
    """include/idkpt.h enum idkpt_denoise_route: spacing 1, 2, 4 staged in LDS, 8 and up fetched from memory"""
    return ROUTE_TILED if (1 << iteration) <= 4 else ROUTE_DIRECT


def inv_sigma2(sigma, i):
    """1 / (s * s), s = sigma * 2^-i, in binary32 (the scaling is exact)"""
    with np.errstate(all="ignore"):
        s = F(np.ldexp(F(sigma), -int(i)))
        return F(1.0) / F(s * s)


def floor_albedo(a):
    return np.fmax(a, EPS)                     # fmaxf: a NaN channel acts as eps


def _dist2(u, P, Q):
    d = u[Q] - u[P]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def iteration(c, a, n, s, invC, invA, invN, skip=None):
    """one iteration with tap spacing s; c, a, n: (H, W, 3) float32"""
    H, W = c.shape[:2]
    acc = np.zeros((H, W, 3), F); accW = np.zeros((H, W), F)
    one = F(1.0)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):                # the outer loop
            for dx in range(-2, 3):            # the inner loop
                y0, y1 = max(0, -s * dy), min(H, H - s * dy)
                x0, x1 = max(0, -s * dx), min(W, W - s * dx)
                if y0 >= y1 or x0 >= x1:
                    continue                   # every such tap is outside the image: skipped
                P = (slice(y0, y1), slice(x0, x1)); Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                h = F(K[dx + 2] * K[dy + 2])
                w = ((h * (one / (one + _dist2(c, P, Q) * invC))) * (one / (one + _dist2(a, P, Q) * invA))) * (one / (one + _dist2(n, P, Q) * invN))
                ok = w > 0                     # false for NaN and for 0
                if skip is not None:
                    ok = ok & ~skip[Q]
                acc[P] = np.where(ok[..., None], acc[P] + c[Q] * w[..., None], acc[P])
                accW[P] = np.where(ok, accW[P] + w, accW[P])
        return np.where((accW == 0)[..., None], c, acc / accW[..., None]).astype(F)


def denoise(result, albedo, normal, Iterations=5, ColorSigma=8.0, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1, skip=None):
    """(H, W, 4) float32: rgb as the contract defines it, alpha 1.0.  result, albedo, normal: (H, W, >= 3) float32 images as accumulated."""
    c = np.ascontiguousarray(np.asarray(result, F)[..., :3]); a = np.ascontiguousarray(np.asarray(albedo, F)[..., :3]); n = np.ascontiguousarray(np.asarray(normal, F)[..., :3])
    with np.errstate(all="ignore"):
        if DemodulateAlbedo:
            c = (c / floor_albedo(a)).astype(F)
        invA, invN = inv_sigma2(AlbedoSigma, 0), inv_sigma2(NormalSigma, 0)
        for i in range(int(Iterations)):
            c = iteration(c, a, n, 1 << i, inv_sigma2(ColorSigma, i), invA, invN, skip)
        if DemodulateAlbedo:
            c = (c * floor_albedo(a)).astype(F)
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


def random_images(W, H, seed=0):
    """Result, Albedo, Normal (H, W, 4) float32: smooth shading plus noise, albedo with channels at 0 and below eps in places, unit-ish normals in a few orientations"""
    rng = np.random.default_rng(1000 * seed + 31 * W + H)
    y, x = np.mgrid[0:H, 0:W].astype(F)
    albedo = np.empty((H, W, 4), F); normal = np.empty((H, W, 4), F); result = np.empty((H, W, 4), F)
    block = ((x // 5).astype(int) + 2 * (y // 4).astype(int)) % 4
    palette = np.array([[0.8, 0.7, 0.6], [0.2, 0.5, 0.9], [0.0, 0.0005, 0.3], [0.95, 0.05, 0.0002]], F)      # channels at 0 and below eps
    normals = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [-0.70710677, 0.70710677, 0.0]], F)
    albedo[..., :3] = palette[block] + (rng.random((H, W, 3)) * 0.01).astype(F) * (palette[block] > 0.01)
    normal[..., :3] = normals[(block + (y // 7).astype(int)) % 4]
    shade = (0.4 + 0.3 * np.sin(x * F(0.37)) * np.cos(y * F(0.23))).astype(F)
    result[..., :3] = albedo[..., :3] * shade[..., None] * (0.5 + rng.random((H, W, 3))).astype(F) + (rng.random((H, W, 3)) * 0.02).astype(F)
    albedo[..., 3] = 1.0; normal[..., 3] = 1.0; result[..., 3] = 1.0
    return result, albedo, normal


NONFINITE = [("nan", F(np.nan)), ("+inf", F(np.inf)), ("-inf", F(-np.inf)), ("flt_max", np.finfo(F).max)]


def plant(images, which, value, pos, channel=1):
    """a copy of (result, albedo, normal) with `value` in one channel of image `which` (0, 1, 2) at pos = (x, y)"""
    out = [im.copy() for im in images]
    out[which][pos[1], pos[0], channel] = value
    return tuple(out)


def settings(Iterations, DemodulateAlbedo, ColorSigma=0.5, AlbedoSigma=0.2, NormalSigma=0.5):
    return dict(Iterations=Iterations, ColorSigma=ColorSigma, AlbedoSigma=AlbedoSigma, NormalSigma=NormalSigma, DemodulateAlbedo=DemodulateAlbedo)


# (W, H, settings): every shape of SHAPES; 5 x 3 with 5 iterations (from spacing 4 on every non-centre tap is outside); 70 x 41 with 1, 3 and 6 iterations (tile seams in
# both axes: TILED only, every tiled spacing, both routes); DemodulateAlbedo 0 and 1; Iterations 1 and 8
CASES = [
    (1, 1, settings(1, 1)), (1, 1, settings(8, 0)), (5, 3, settings(5, 1)), (16, 16, settings(2, 0)), (16, 16, settings(1, 1)), (17, 16, settings(3, 1)), (16, 17, settings(3, 0)),
    (37, 23, settings(4, 1)), (37, 23, settings(8, 0)), (70, 41, settings(1, 0)), (70, 41, settings(3, 1)), (70, 41, settings(6, 1)), (70, 41, dict(DEFAULTS)),
]
PLANT_POS = (18, 11)                          # in the 37 x 23 image: interior, not on a tile seam's first column
PLANT_SETTINGS = [settings(4, 0), settings(4, 1)]      # spacing 1, 2, 4 (tiled) and 8 (direct)
