"""The noise estimate of include/idkpt.h ("noise estimate") restated in numpy, in binary32, operation for operation: the fold of a sample's luminance into the
moments (m1, m2) FinalDraw keeps, the per-pixel relative standard error, the pairwise tree over an 8 x 8 tile and the summary record.  Independent of the library: nothing
is imported from it, the text of the header is the only source.  Compared with == on bit patterns against a host build of idkengine_amd/csrc/noise_texel.hpp
(tests/test_noise_ref.py) and against the device (tests/test_gpu_noise.py).

Every array is float32 and every scalar is wrapped in np.float32 before it meets one, so numpy rounds each + - * / and sqrt to binary32 exactly once, as the library does
under -ffp-contract=off."""
import numpy as np

F = np.float32
TILE = 8
DEFAULTS = dict(Epsilon=1e-2, Threshold=0.05)
LUMA = (F(0.2126), F(0.7152), F(0.0722))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def luminance(nr):
    """L = (0.2126f * nr.x + 0.7152f * nr.y) + 0.0722f * nr.z of an (..., >= 3) float32 array"""
    nr = np.asarray(nr, F)
    with np.errstate(all="ignore"):
        return (LUMA[0] * nr[..., 0] + LUMA[1] * nr[..., 1]) + LUMA[2] * nr[..., 2]


def weight(accumulated):
    """FinalDraw's weight of the sample that finds `accumulated` samples in the slot"""
    return F(1.0) / (F(accumulated) + F(1.0))


def mix(x, y, a):
    """GLSL mix as the library writes it: x * (1 - a) + y * a"""
    with np.errstate(all="ignore"):
        return x * (F(1.0) - a) + y * a


def fold(m1, m2, nr, accumulated):
    """one sample: (m1, m2) after folding the luminance of radiance image nr with the weight of `accumulated`"""
    L = luminance(nr); w = weight(accumulated)
    with np.errstate(all="ignore"):
        return mix(m1, L, w), mix(m2, L * L, w)


def moments(samples, m1=None, m2=None, accumulated=0):
    """the moments after folding `samples` (a sequence of (H, W, >= 3) radiance images) in order, starting from (m1, m2) (zeros) with `accumulated` samples in the slot"""
    shape = np.asarray(samples[0]).shape[:2]
    m1 = np.zeros(shape, F) if m1 is None else np.asarray(m1, F).copy()
    m2 = np.zeros(shape, F) if m2 is None else np.asarray(m2, F).copy()
    for k, nr in enumerate(samples):
        m1, m2 = fold(m1, m2, nr, accumulated + k)
    return m1, m2


def moments_image(m1, m2):
    """what idkptDownloadMoments returns: (m1, m2, 0, 1)"""
    out = np.zeros(m1.shape + (4,), F)
    out[..., 0] = m1; out[..., 1] = m2; out[..., 3] = 1.0
    return out


def pixel_error(m1, m2, n, epsilon):
    """e = sqrtf(fmaxf(m2 - m1 * m1, 0) / (float)(n - 1)) / (fmaxf(m1, 0) + Epsilon); +Inf where a moment is not finite"""
    assert n >= 2
    m1 = np.asarray(m1, F); m2 = np.asarray(m2, F)
    with np.errstate(all="ignore"):
        var = np.fmax(m2 - m1 * m1, F(0.0))
        e = np.sqrt(var / F(n - 1)) / (np.fmax(m1, F(0.0)) + F(epsilon))
    return np.where(np.isfinite(m1) & np.isfinite(m2), e, F(np.inf)).astype(F)


def tile_map(e):
    """(tilesY, tilesX, 2) float32 of (mean, max) from the (H, W) error image: positions j = (y & 7) * 8 + (x & 7), outside counting as 0, the tree j ^ 1, 2, 4, 8, 16, 32"""
    H, W = e.shape
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    padded = np.zeros((ty * TILE, tx * TILE), F); padded[:H, :W] = e
    inside = np.zeros((ty * TILE, tx * TILE), bool); inside[:H, :W] = True
    split = lambda a: a.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE)   # noqa: E731  (j = row-in-tile * 8 + column-in-tile)
    v = split(padded); count = split(inside).sum(axis=2)
    mx = v.max(axis=2)                                   # e >= 0 and never NaN, the outside positions hold 0: the maximum over the inside pixels
    j = np.arange(TILE * TILE)
    with np.errstate(all="ignore"):
        for mask in (1, 2, 4, 8, 16, 32):
            v = v + v[..., j ^ mask]
        mean = v[..., 0] / count.astype(F)
    return np.stack([mean.astype(F), mx.astype(F)], axis=2)


def summary(tiles, threshold, n):
    """the record idkptEstimateNoise leaves: TilesAbove, MaxTileMean, Tiles, Samples"""
    mean = tiles[..., 0]
    return {"TilesAbove": int((mean > F(threshold)).sum()), "MaxTileMean": F(mean.max()), "Tiles": int(mean.size), "Samples": int(n)}


def estimate(m1, m2, n, Epsilon=DEFAULTS["Epsilon"], Threshold=DEFAULTS["Threshold"]):
    """(tiles, summary) of idkptEstimateNoise on the moments (m1, m2) after n samples"""
    tiles = tile_map(pixel_error(m1, m2, n, Epsilon))
    return tiles, summary(tiles, Threshold, n)


def same_summary(a, b):
    return (a["TilesAbove"], a["Tiles"], a["Samples"]) == (b["TilesAbove"], b["Tiles"], b["Samples"]) and same(F(a["MaxTileMean"]), F(b["MaxTileMean"]))
