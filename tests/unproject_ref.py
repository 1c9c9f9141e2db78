"""Reference of the equirectangular unprojection the library runs on the device (idkptUnprojectSky; csrc/unproject_texel.hpp, csrc/kernels_unproject.hpp), written in numpy
from SkyBoxManager.LoadSkyBoxEquirectangular (Source/Render/SkyBoxManager.cs:115-146) and Shaders/UnprojectEquirectangular/compute.glsl (main, SampleSphericalMap,
SrgbToLinear; GetWorldSpaceDirection of include/Math.glsl:17-39), independently of the kernels.

unproject(bits, S, dtype):
  np.float32   the shader's operation sequence, every written operation rounded once to binary32 (what unproject_texel.hpp restates);
  np.float64   the same formula in binary64 with the constants as the shader writes them: the yardstick the binary32 executions (the reference's shader on llvmpipe,
               tests/golden/unproject/cases.npz; this restatement; the host build of the header; the device) are measured against.
Conventions: uv = (texel + 0.5) / S, ndc = uv * 2 - 1; normalize(v) = v * (1 / sqrt(dot(v, v))), dot summed left to right; atan2 / asin from numpy; the sampler has the GL
defaults (REPEAT, one level, magnification LINEAR): f = u * size - 0.5, i0 = floor(f), weight f - i0, texels i0 and i0 + 1 modulo the size (wrap="clamp" evaluates the
clamped variant, which the tests show to be wrong); mix(x, y, a) = x * (1 - a) + y * a; SrgbToLinear a selection by c < 0.04045.
Storage: the panorama is uploaded as RGBA16F bits, (H, W, 4) uint16 — rne_half, round to nearest even with subnormals, the library's saturation at 65504 (pack) —, the cube
is stored by rtz_half (round toward zero, saturating, subnormals: bloom's rule).

CASES are the fixture's; input_image(case) its inputs."""
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "unproject", "cases.npz")

# (W, H, S, channels, faceSize argument of idkptUnprojectSky: 0 = W // 4)
CASES = (
    (16, 8, 4, 3, 0),       # even S (no texel of it has a footprint across the panorama's edge: wrapping_texels)
    (20, 10, 5, 3, 0),      # odd S: the centre column of -X and the centres of +-Y (atan of a zero z)
    (18, 9, 4, 3, 0),       # W no multiple of 4
    (24, 16, 6, 3, 0),      # not 2:1
    (32, 16, 9, 3, 9),      # an explicit size: partial 8 x 8 groups, S != W / 4
    (64, 32, 16, 4, 0),     # four channels, random alpha
    (16, 8, 12, 3, 12),     # S beyond W / 4: with S = W / 4 no footprint of an ordinary texel crosses the panorama's edge (see wrapping_texels); at S = 12 many do, in both axes
)
HALF_SUBNORMAL = 2.0 ** -24
INV_ATAN = (0.1591, 0.3183)


def _lcg(n, seed):
    """n values in [0, 1): multiples of 2^-16 from a 32-bit linear congruential sequence (the same on every platform)."""
    out = np.empty(n, np.float64); s = seed
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = (s >> 16) / 65536.0
    return out


_IMAGES = {}


def input_image(case):
    """(H, W, channels) float32 from a seeded LCG.  Per texel one of eight kinds, chosen by its own draw (k), the colour channels from three more (r):
    k < .08 zeros | < .12 the constant 0.04045f itself | < .30 values on both sides of it, [0.03, 0.05) | < .38 small negatives, (-0.01, 0] | < .46 values whose half
    is subnormal, [0, 6e-5) | < .58 exact half ties (a half in [0, 4) plus half its spacing: representable in binary32) | < .66 up to 6e4 | else ordinary HDR, [0, 4.5).
    Alpha of a four-channel case: [0, 1) at random.  Nothing beyond 65504; finite."""
    if case in _IMAGES:
        return _IMAGES[case].copy()
    W, H, _, ch, _ = case
    d = _lcg(W * H * 5, 4711 + 13 * W + H).reshape(H, W, 5)
    k = d[..., 0:1]; r = d[..., 1:4]
    h = (r * 4.0).astype(np.float16)
    spacing = np.spacing(h).astype(np.float64)
    ties = h.astype(np.float64) + spacing / 2
    rgb = np.select([k < .08, k < .12, k < .30, k < .38, k < .46, k < .58, k < .66],
                    [np.zeros_like(r), np.full_like(r, np.float64(np.float32(0.04045))), 0.03 + 0.02 * r, -0.01 * r, 6e-5 * r, ties, 6e4 * r], 4.5 * r)
    img = np.concatenate([rgb, d[..., 4:5]], axis=2)[..., :ch].astype(np.float32)
    assert np.isfinite(img).all() and np.abs(img).max() < 65504
    assert (ties.astype(np.float32).astype(np.float64) == ties).all()
    _IMAGES[case] = img
    return img.copy()


# ---- storage
def rne_half(v):
    """float array -> binary16 bits, round to nearest even, subnormal halves produced; a finite value whose nearest half is infinite -> +-65504 (the library's deviation)."""
    v = np.asarray(v)
    with np.errstate(over="ignore"):
        bits = v.astype(np.float16).view(np.uint16).copy()
    inf = ((bits & 0x7FFF) == 0x7C00) & np.isfinite(v)
    bits[inf] -= 1
    return bits


def rtz_half(v):
    """float array (binary32 or binary64) -> binary16 bits, rounded toward zero; a finite value beyond 65504 -> 65504 (0x7BFF); subnormal halves are produced."""
    v = np.asarray(v)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    bits = h.view(np.uint16).copy()
    away = (np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))) & np.isfinite(v)
    bits[away] -= 1
    return bits


def half_values(bits, dtype):
    return np.ascontiguousarray(bits).view(np.float16).astype(dtype)   # exact


def is_half(v):
    """every float32 of v is exactly representable in binary16"""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore"):
        return np.isfinite(v) & (v.astype(np.float16).astype(np.float32) == v)


def pack(img):
    """Upload2D into the R16G16B16A16Float texture: (H, W, 3 | 4) float32 -> (H, W, 4) uint16, alpha 1.0 for three channels"""
    H, W, ch = img.shape
    out = np.full((H, W, 4), 0x3C00, np.uint16)
    out[..., :ch] = rne_half(img)
    return out


# ---- the shader
def directions(S, dtype):
    """GetWorldSpaceDirection(ndc, face) for the 6 x S x S texels: (6, S, S, 3)"""
    dt = dtype
    c = ((np.arange(S).astype(dt) + dt(0.5)) / dt(S)) * dt(2.0) - dt(1.0)
    x = np.broadcast_to(c[None, :], (S, S)); y = np.broadcast_to(c[:, None], (S, S))
    one = np.ones((S, S), dt)
    faces = [(one, -y, -x), (-one, -y, x), (x, one, y), (x, -one, -y), (x, -y, one), (-x, -y, -one)]
    out = np.empty((6, S, S, 3), dt)
    for f, (vx, vy, vz) in enumerate(faces):
        inv = dt(1.0) / np.sqrt(vx * vx + vy * vy + vz * vz)
        out[f, ..., 0] = vx * inv; out[f, ..., 1] = vy * inv; out[f, ..., 2] = vz * inv
    return out


def seam_masks(S):
    """(column, poles): the texels whose atan GLSL leaves to the driver.  column: the centre column of face -X (z == +0 exactly, x < 0: +pi in C, -pi for a driver that
    drops the zero's sign); poles: the centres of faces +Y and -Y (x == 0 and z == 0: `atan(y, x)` is UNDEFINED there in GLSL; C returns +-0, Mesa's lowering
    +-3 pi / 4).  Both exist at odd S only.  (The left half of the centre row of +-Y has z == +-0 and x < 0 as well; C's signs give +pi on +Y and -pi on -Y, the two
    branches differ there only by exchanging two nearly equal weights, and those texels are compared like every other.)"""
    d = directions(S, np.float32)
    zero = (d[..., 2] == 0) & (d[..., 0] <= 0)
    column = np.zeros_like(zero); column[1] = zero[1]
    poles = zero & (d[..., 0] == 0)
    return column, poles


def seam_mask(S):
    column, poles = seam_masks(S)
    return column | poles


def spherical_uv(d, dtype, atan_override=None):
    dt = dtype
    at = np.arctan2(d[..., 2], d[..., 0]).astype(dt)
    if atan_override is not None:
        m, value = atan_override
        at = np.where(m, np.asarray(value).astype(dt), at)
    u = at * dt(INV_ATAN[0]) + dt(0.5)
    v = np.arcsin(d[..., 1]).astype(dt) * dt(INV_ATAN[1]) + dt(0.5)
    return u, v


def taps(u, size, dtype, wrap="repeat"):
    """(i0, i1, weight of i1)"""
    dt = dtype
    f = u * dt(size) - dt(0.5)
    f0 = np.floor(f)
    a = f - f0
    i0 = f0.astype(np.int64); i1 = i0 + 1
    if wrap == "repeat":
        return i0 % size, i1 % size, a
    return np.clip(i0, 0, size - 1), np.clip(i1, 0, size - 1), a


def srgb_to_linear(c, dtype):
    dt = dtype
    with np.errstate(invalid="ignore"):
        higher = np.power((c + dt(0.055)) / dt(1.055), dt(2.4)).astype(dt)
    lower = c / dt(12.92)
    return np.where(c < dt(0.04045), lower, higher)


def shift_ulps(a, k):
    """every element of the float array moved k units in the last place (k < 0: toward -inf)"""
    a = np.array(a)
    for _ in range(abs(k)):
        a = np.nextafter(a, a.dtype.type(np.inf if k > 0 else -np.inf))
    return a


def unproject(bits, S, dtype, wrap="repeat", atan_override=None, uv_ulps=(0, 0)):
    """the value imageStore receives for every texel of the cube, (6, S, S, 4) of dtype, and the largest |tap| per texel and channel (6, S, S, 4) float64.
    uv_ulps: u and v moved that many units in the last place before the filter (what another atan2f / asinf may return)"""
    dt = dtype
    H, W = bits.shape[:2]
    tex = half_values(bits, dt)
    u, v = spherical_uv(directions(S, dt), dt, atan_override)
    u, v = shift_ulps(u, uv_ulps[0]), shift_ulps(v, uv_ulps[1])
    x0, x1, ax = taps(u, W, dt, wrap); y0, y1, ay = taps(v, H, dt, wrap)
    a, b, c, d = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    ax = ax[..., None]; ay = ay[..., None]
    mix = lambda p, q, w: p * (dt(1.0) - w) + q * w
    col = mix(mix(a, b, ax), mix(c, d, ax), ay)
    out = np.empty_like(col)
    out[..., :3] = srgb_to_linear(col[..., :3], dt)
    out[..., 3] = col[..., 3]
    big = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d))).astype(np.float64)
    return out.astype(dt), big


def scale_of(big):
    """what an error of a texel and channel is measured in: the binary64 SrgbToLinear of the largest |tap| (alpha: the tap itself), at least one half subnormal"""
    s = big.copy()
    s[..., :3] = srgb_to_linear(big[..., :3], np.float64)
    return np.maximum(s, HALF_SUBNORMAL)


def seam_branches(S):
    """[(mask, atan values)]: every combination a driver may return at the seam texels — the column +pi or -pi, the poles any multiple of pi / 4 in [-pi, pi] (what a
    lowering that resolves 0 / 0 into some octant returns; C's 0 is one of them)"""
    column, poles = seam_masks(S)
    out = []
    for k in range(-4, 5):
        at = np.zeros(column.shape); at[column] = np.pi if k >= 0 else -np.pi; at[poles] = k * np.pi / 4
        out.append((column | poles, at))
    return out


def evaluate64(bits, S):
    """[(T, scale)] in binary64: the first entry follows numpy / C at the seam texels, the others put every allowed atan there (odd S only)"""
    T, big = unproject(bits, S, np.float64)
    out = [(T, scale_of(big))]
    if seam_mask(S).any():
        for ov in seam_branches(S):
            T, big = unproject(bits, S, np.float64, atan_override=ov)
            out.append((T, scale_of(big)))
    return out


def wrapping_texels(W, H, S):
    """(6, S, S) bool: texels whose footprint crosses an edge of the panorama, i. e. where REPEAT and CLAMP_TO_EDGE differ.  With S = W / 4 these are the seam texels only:
    the texel centres next to the seam lie atan(2 / S) > 2 / S from it, but a footprint wraps only within pi / W = 0.79 / S of it."""
    u, v = spherical_uv(directions(S, np.float64), np.float64)
    out = np.zeros(u.shape, bool)
    for c, n in ((u, W), (v, H)):
        r0, r1, _ = taps(c, n, np.float64, "repeat"); c0, c1, _ = taps(c, n, np.float64, "clamp")
        out |= (r0 != c0) | (r1 != c1)
    return out


def scaled_err(X, T, scale, mask=None):
    """max over the (unmasked) texels and channels of |X - T| / scale"""
    e = np.abs(np.asarray(X, np.float64) - T) / scale
    if mask is not None:
        e = e[~mask]
    return float(e.max())


def halves_within(h_bits, T, scale, b):
    """rtz(T - b scale) <= h <= rtz(T + b scale), compared as values"""
    h = half_values(np.asarray(h_bits), np.float64)
    lo = half_values(rtz_half(T - b * scale), np.float64); hi = half_values(rtz_half(T + b * scale), np.float64)
    return (lo <= h) & (h <= hi)


# ---- texture(samplerCube, dir) on the finished seamless cube: the arithmetic of SampleSky (csrc/pt_kernels.hpp) in binary64
def _fold(S, face, x, y):
    sc, tc = 2 * x + 1 - S, 2 * y + 1 - S
    px, py, pz = [(S, -tc, -sc), (-S, -tc, sc), (sc, S, tc), (sc, -S, -tc), (sc, -tc, S), (-sc, -tc, -S)][face]
    m = face >> 1
    ox = m != 0 and abs(px) > S; oy = m != 1 and abs(py) > S; oz = m != 2 and abs(pz) > S
    if not (ox or oy or oz):
        return face, x, y
    inn = S - 1
    if m == 0: px = inn if px > 0 else -inn
    elif m == 1: py = inn if py > 0 else -inn
    else: pz = inn if pz > 0 else -inn
    if oz: pz = S if pz > 0 else -S; face = 4 if pz > 0 else 5
    elif oy: py = S if py > 0 else -S; face = 2 if py > 0 else 3
    else: px = S if px > 0 else -S; face = 0 if px > 0 else 1
    sc, tc = [(-pz, -py), (pz, -py), (px, pz), (px, -pz), (px, -py), (-px, -py)][face]
    return face, (sc + S - 1) // 2, (tc + S - 1) // 2


def sample_cube(faces, dirs):
    """faces (6, S, S, 4) float, dirs (n, 3): (n, 3) float64 and the largest |tap| per sample"""
    S = faces.shape[1]
    f64 = np.asarray(faces, np.float64)
    out = np.zeros((len(dirs), 3)); big = np.zeros(len(dirs))
    for n, d in enumerate(np.asarray(dirs, np.float64)):
        ax, ay, az = np.abs(d)
        if ax >= ay and ax >= az: face, sc, tc, ma = (0, -d[2], -d[1], ax) if d[0] >= 0 else (1, d[2], -d[1], ax)
        elif ay >= az: face, sc, tc, ma = (2, d[0], d[2], ay) if d[1] >= 0 else (3, d[0], -d[2], ay)
        else: face, sc, tc, ma = (4, d[0], -d[1], az) if d[2] >= 0 else (5, -d[0], -d[1], az)
        fx = 0.5 * (sc / ma + 1.0) * S - 0.5; fy = 0.5 * (tc / ma + 1.0) * S - 0.5
        x0 = int(min(max(np.floor(fx), -1.0), S - 1)); y0 = int(min(max(np.floor(fy), -1.0), S - 1))
        wx, wy = fx - np.floor(fx), fy - np.floor(fy)
        t = [None] * 4
        for k in range(4):
            x, y = x0 + (k & 1), y0 + (k >> 1)
            if (x < 0 or x >= S) and (y < 0 or y >= S):
                continue
            f2, x, y = _fold(S, face, x, y)
            t[k] = f64[f2, y, x, :3]
        have = [v for v in t if v is not None]
        if len(have) < 4:
            t = [v if v is not None else sum(have) / 3.0 for v in t]
        mix = lambda p, q, w: p * (1.0 - w) + q * w
        out[n] = mix(mix(t[0], t[1], wx), mix(t[2], t[3], wx), wy)
        big[n] = max(np.abs(v).max() for v in t)
    return out, big


def cube_dirs(n, seed):
    """n fixed directions (float32, not normalised: cube lookups do not need it), none with two equal largest components"""
    r = _lcg(n * 3, seed).reshape(n, 3) * 2.0 - 1.0
    r[np.abs(r).max(axis=1) < 0.05] += 0.5
    return r.astype(np.float32)


def load_fixture():
    return np.load(FIXTURE)
