"""Reference of the bloom the library runs on the device (idkptBloom; csrc/bloom_texel.hpp, csrc/kernels_bloom.hpp), written in numpy from the arithmetic of
Shaders/Bloom/compute.glsl (main, Downsample, Upsample, Prefilter) and the sizes and bindings of Source/Render/Bloom.cs:56-147, independently of the kernels.

Every function takes dtype:
  np.float32   the shader's operation sequence, every written operation rounded once to binary32 (what bloom_texel.hpp restates: compared bit for bit);
  np.float64   the same formula in binary64 with the constants as the shader writes them: the yardstick the binary32 executions (the reference's shader on llvmpipe,
               tests/golden/bloom/chain.npz; this restatement; the device) are measured against.
Conventions (GLSL leaves the filter's arithmetic to the implementation; hence a measured bound, tests/test_bloom_ref.py): textureLod / textureLodOffset = linear
filter, clamp to edge, explicit level; uv = (texel + 0.5) / size of the written level; f = u * size - 0.5 + offset, i0 = floor(f), weight f - i0, texels i0 and
i0 + 1 with clamped indices; mix(x, y, a) = x * (1 - a) + y * a, x first, then y.
Storage: levels are RGBA16F bits, (h, w, 4) uint16, alpha 0x3C00.  rtz_half is the header's rule: round toward zero, finite overflow -> 65504, subnormals produced,
+-Inf kept, NaN -> sign | 0x7E00.
Non-finite texels (include/idkpt.h "Non-finite and extreme texels"; tests/adversarial_pixels.py): min / max are GLSL's definitions, y < x ? y : x and x < y ? y : x
(_min / _max: Prefilter turns a NaN channel into MaxColor), and the filter's mix is evaluated as written, Inf * 0 = NaN under a weight of exactly 0.

down_pass / up_pass / expand run ONE pass from given input bits; chain runs everything from an image.  CASES are the fixture's; input_image(case) its inputs."""
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "bloom", "chain.npz")

# (W, H, Threshold, MaxColor, MinusLods).  The reference's defaults are 1.5, 3.8, 3 (Bloom.cs:12-13, 46)
CASES = (
    (64, 48, 1.0, 3.0e5, 3),      # an even chain: 32 x 24, 16 x 12, 8 x 6; MaxColor so large that levels exceed 65504 (saturating stores)
    (37, 23, 1.5, 3.8, 3),        # floor sizes (18 x 11, 9 x 5) and non-half weights; the two-level minimum reached by MinusLods
    (40, 6, 1.5, 3.8, 0),         # levels one texel high, down to 1 x 1: 20 x 3, 10 x 1, 5 x 1, 2 x 1, 1 x 1
    (2, 2, 1.5, 3.8, 3),          # the smallest frame: 1 x 1 and 1 x 1
    (261, 141, 1.5, 3.8, 3),      # several workgroups and tile seams, odd at most levels: 130 x 70, 65 x 35, 32 x 17, 16 x 8, 8 x 4
)
KNEE = 0.2


def sizes(W, H, minus_lods):
    """(levels, [(w, h) of level 0 .. levels - 1]) — Bloom.SetSize: integer division, then GetMaxMipmapLevel - MinusLods, at least 2."""
    w0, h0 = W // 2, H // 2
    levels = max(int(np.floor(np.log2(max(w0, h0)))) + 1 - minus_lods, 2)
    return levels, [(max(w0 >> l, 1), max(h0 >> l, 1)) for l in range(levels)]


def _lcg(n, seed):
    """n values in [0, 1): multiples of 2^-16 from a 32-bit linear congruential sequence (the same on every platform)."""
    out = np.empty(n, np.float64); s = seed
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = (s >> 16) / 65536.0
    return out


_IMAGES = {}


def input_image(case):
    """(H, W, 4) float32 from a seeded LCG: colours in [0, 4.5) — brightness below Threshold - Knee, inside the knee, above it and above the default MaxColor —; one
    pixel in ten exactly zero; the right third three times as bright (it survives the second Prefilter of level 1);
    the left third a smooth grey ramp Threshold - Knee + [0, 0.012) (Prefilter's rq is tiny there: level 0 lands on subnormal halves);
    the bottom right quarter of a case with MaxColor > 1e4 multiplied by 6e4 (level values beyond 65504).  Alpha 1.  Finite."""
    if case in _IMAGES:
        return _IMAGES[case].copy()
    W, H, thr, maxc, _ = case
    r = _lcg(W * H * 4, 2024 + 7 * W + H).reshape(H, W, 4)
    img = np.ones((H, W, 4), np.float64)
    img[..., :3] = r[..., :3] * 4.5
    img[..., :3][r[..., 3] < 0.1] = 0.0
    x = np.arange(W, dtype=np.float64)[None, :] / W; y = np.arange(H, dtype=np.float64)[:, None] / H
    n = W // 3
    if n >= 2:
        img[:, :n, :3] = ((thr - KNEE) + 0.012 * (x[:, :n] * 3.0) * (0.25 + 0.75 * y))[..., None] * np.array([1.0, 0.7, 0.4])
    img[:, W - n:, :3] *= 3.0                                      # the right third bright enough to pass both prefilters (levels 0 and 1)
    if maxc > 1e4:
        img[H // 2:, W // 2:, :3] *= 6.0e4
    out = img.astype(np.float32)
    assert np.isfinite(out).all()
    _IMAGES[case] = out
    return out.copy()


# ---- storage
def rtz_half(v):
    """float array (binary32 or binary64) -> binary16 bits, rounded toward zero; a finite value beyond 65504 -> 65504 (0x7BFF); subnormal halves are produced;
    +-Inf stays; a NaN becomes sign | 0x7E00 whatever its payload (f32_to_f16_rtz)."""
    v = np.asarray(v)
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(np.float16)                                   # round to nearest even, overflow to Inf
        away = (np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))) & np.isfinite(v)
    bits = h.view(np.uint16).copy()
    bits[away] -= 1                                                # one step toward zero (sign-magnitude; Inf - 1 = 65504)
    nan = np.isnan(v)
    bits[nan] = np.where(np.signbit(v[nan]), 0xFE00, 0x7E00).astype(np.uint16)
    return bits


def half_values(bits, dtype):
    return np.ascontiguousarray(bits).view(np.float16).astype(dtype)   # exact


def store(rgb):
    """imageStore(ImgResult, p, vec4(result, 1.0)) to an RGBA16F level: (h, w, 4) uint16"""
    out = np.full(rgb.shape[:2] + (4,), 0x3C00, np.uint16)
    out[..., :3] = rtz_half(rgb)
    return out


# ---- sampling
def _coords(n, dt):
    return (np.arange(n).astype(dt) + dt(0.5)) / dt(n)


def _axis(u, size, off, dt):
    f = u * dt(size) - dt(0.5) + dt(off)
    i0f = np.floor(f)
    i0 = i0f.astype(np.int64)
    return np.clip(i0, 0, size - 1), np.clip(i0 + 1, 0, size - 1), f - i0f


def _tap(src, u, v, ox, oy, dt):
    """textureLodOffset(src, uv, lod, ivec2(ox, oy)).rgb for the grid v x u; src (h, w, 3) of dtype dt"""
    h, w = src.shape[:2]
    xa, xb, ax = _axis(u, w, ox, dt); ya, yb, ay = _axis(v, h, oy, dt)
    ax = ax[None, :, None]; ay = ay[:, None, None]
    a = src[ya[:, None], xa[None, :]]; b = src[ya[:, None], xb[None, :]]; c = src[yb[:, None], xa[None, :]]; d = src[yb[:, None], xb[None, :]]
    mix = lambda p, q, t: p * (dt(1.0) - t) + q * t
    return mix(mix(a, b, ax), mix(c, d, ax), ay)


def _downsample(src, dw, dh, dt):
    u, v = _coords(dw, dt), _coords(dh, dt)
    t = lambda ox, oy: _tap(src, u, v, ox, oy, dt)
    center = t(0, 0); yellowUpRight = t(0, 2); yellowDownLeft = t(-2, 0); greenDownRight = t(2, 0); blueDownLeft = t(0, -2)
    yellow = t(-2, 2); yellow = yellow + yellowUpRight; yellow = yellow + center; yellow = yellow + yellowDownLeft
    green = yellowUpRight; green = green + t(2, 2); green = green + greenDownRight; green = green + center
    blue = center; blue = blue + greenDownRight; blue = blue + t(2, -2); blue = blue + blueDownLeft
    lila = yellowDownLeft; lila = lila + center; lila = lila + blueDownLeft; lila = lila + t(-2, -2)
    red = t(-1, 1); red = red + t(1, 1); red = red + t(1, -1); red = red + t(-1, -1)
    return (red * dt(0.5) + (yellow + green + blue + lila) * dt(0.125)) * dt(0.25)


def _upsample(src, dw, dh, dt):
    u, v = _coords(dw, dt), _coords(dh, dt)
    t = lambda ox, oy: _tap(src, u, v, ox, oy, dt)
    r = t(-1, 1) * dt(1.0); r = r + t(0, 1) * dt(2.0); r = r + t(1, 1) * dt(1.0)
    r = r + t(-1, 0) * dt(2.0); r = r + t(0, 0) * dt(4.0); r = r + t(1, 0) * dt(2.0)
    r = r + t(-1, -1) * dt(1.0); r = r + t(0, -1) * dt(2.0); r = r + t(1, -1) * dt(1.0)
    return r / dt(16.0)


def _min(x, y):
    """GLSL's min by its definition, y < x ? y : x (bloomt::minf): a NaN x is returned, a NaN y is dropped"""
    return np.where(y < x, y, x)


def _max(x, y):
    """GLSL's max by its definition, x < y ? y : x (bloomt::maxf)"""
    return np.where(x < y, y, x)


def _prefilter(c, max_color, threshold, dt):
    knee = dt(np.float32(KNEE)) if dt is np.float32 else dt(KNEE)
    max_color, threshold = dt(np.float32(max_color)), dt(np.float32(threshold))      # the settings are binary32 values
    c = _min(max_color, c)                                                           # min(vec3(maxColor), color)
    b = _max(_max(c[..., 0], c[..., 1]), c[..., 2])
    cx, cy, cz = threshold - knee, knee * dt(2.0), dt(0.25) / knee
    rq = _min(_max(b - cx, dt(0.0)), cy)
    rq = (rq * rq) * cz
    s = _max(rq, b - threshold) / _max(b, dt(0.0001))
    return c * s[..., None]


def _check(a, dt):
    assert a.dtype == dt, (a.dtype, dt)
    return a


# ---- one pass from given inputs; all return the value imageStore receives, (h, w, 3) of dtype dt
def down_pass0(img, size, threshold, max_color, dt):
    """Down pass 0: Downsample(the image, Lod 0), Prefilter.  img (H, W, 4) float32; size = (w0, h0)."""
    src = np.asarray(img)[..., :3].astype(dt)
    return _check(_prefilter(_downsample(src, size[0], size[1], dt), max_color, threshold, dt), dt)


def down_pass(prev_bits, size, dt, prefilter=None):
    """Down pass l >= 1: Downsample(down level l - 1).  prev_bits (h, w, 4) uint16; size of level l.  prefilter = (threshold, max_color) for l = 1: Bloom.cs uploads
    Lod = currentWriteLod - 1 = 0 for that pass, and the shader prefilters `if (Lod == 0)` — the reference prefilters twice (the fixture shows it)."""
    r = _downsample(half_values(prev_bits[..., :3], dt), size[0], size[1], dt)
    return _check(r if prefilter is None else _prefilter(r, prefilter[1], prefilter[0], dt), dt)


def up_pass(up_bits, down_bits, size, dt):
    """The pass that writes up level l: Upsample(up_bits = level l + 1 of the up chain — of the down chain in the first up pass) + one tap of down level l + 1."""
    u, v = _coords(size[0], dt), _coords(size[1], dt)
    return _check(_upsample(half_values(up_bits[..., :3], dt), size[0], size[1], dt) + _tap(half_values(down_bits[..., :3], dt), u, v, 0, 0, dt), dt)


def expand(up0_bits, W, H, dt):
    """texture(Sampler1, (p + 0.5) / (W, H)) of the tonemap shader on up level 0: (H, W, 3)"""
    return _check(_tap(half_values(up0_bits[..., :3], dt), _coords(W, dt), _coords(H, dt), 0, 0, dt), dt)


def chain(img, case, dt):
    """Bloom.Compute: {"down": [bits per level], "up": [bits per level], "down_f": [...], "up_f": [...] (the values in front of the store), "expand": (H, W, 3)},
    with the header's half storage at every level."""
    W, H, thr, maxc, minus = case
    levels, sz = sizes(W, H, minus)
    down_f = [down_pass0(img, sz[0], thr, maxc, dt)]; down = [store(down_f[0])]
    for l in range(1, levels):
        down_f.append(down_pass(down[l - 1], sz[l], dt, (thr, maxc) if l == 1 else None)); down.append(store(down_f[l]))
    up = [None] * (levels - 1); up_f = [None] * (levels - 1)
    for l in range(levels - 2, -1, -1):
        up_f[l] = up_pass(down[l + 1] if l == levels - 2 else up[l + 1], down[l + 1], sz[l], dt); up[l] = store(up_f[l])
    return dict(down=down, up=up, down_f=down_f, up_f=up_f, expand=expand(up[0], W, H, dt))


def load_fixture():
    fx = np.load(FIXTURE)
    assert fx["cases"].shape == (len(CASES), 5)
    return fx


def err(a, b):
    """max |a - b| over R, G, B, in binary64"""
    return float(np.max(np.abs(np.asarray(a)[..., :3].astype(np.float64) - np.asarray(b)[..., :3].astype(np.float64))))
