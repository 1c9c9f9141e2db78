"""Reference of the display pass the library runs on the device (idkptPresent; csrc/kernels_present.hpp), written in numpy from the arithmetic of
Shaders/TonemapAndGammaCorrect/compute.glsl (main, AgX_DS, DualSection, PrimariesToMatrix, ComputeCompressionMatrix, LinearToSrgb, Dither), independently of the kernel.

present(img, settings, add0, add1, dtype) evaluates the value imageStore receives for every texel, (H, W, 4):
  dtype = np.float32   the shader's operation sequence, every written operation rounded once to binary32 (what the kernel restates);
  dtype = np.float64   "the formula's value": the same formula in binary64 with the constants as the shader writes them — the yardstick the binary32 executions (the reference's
                       shader on llvmpipe, tests/golden/present/agx.npz; this restatement; the device) are measured against.
Conventions both restatements share (GLSL leaves them to the implementation; hence a measured bound, tests/test_present_ref.py):
  mat3 is column-major, m[c][r]; M * v sums M[0][r] v.x + M[1][r] v.y + M[2][r] v.z left to right, A * B likewise over k; inverse(mat3) is cofactors divided by the determinant;
  mix(x, y, a) = x * (1 - a) + y * a; dot sums left to right; pow(2, e), exp and pow(x, 1 / 2.4) are the library functions of the dtype.
quantise(x) is the header's rule for IDKPT_DISPLAY_RGBA8: (uint8) rint(min(max(x, 0), 1) * 255.0f) in binary32, alpha 255.
Non-finite texels (include/idkpt.h "Non-finite and extreme texels"; tests/adversarial_pixels.py): every max(.., 0) and clamp is fmaxf / fminf (np.fmax / np.fmin), which drop
a NaN operand, as the kernel's gmax / gmin / gclamp do: a NaN or negative input acts as 0, the NaN of inf - inf inside M * v becomes 0 in the clamp behind DualSection, and every
stored texel is finite; quantise never converts a NaN to an integer.
input_image() / bloom_image() are the fixture's inputs (70 x 40, by formula), CASES its settings."""
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "present", "agx.npz")
W, H = 70, 40

# (Exposure, Saturation, Linear, Peak, Compression, DoTonemapAndSrgbTransform, bloom): TonemapAndGammaCorrect.GpuSettings in its order, + "Sampler1 is bound to bloom_image()"
DEFAULTS = (0.45, 1.06, 0.18, 1.0, 0.1, 1)
CASES = (
    DEFAULTS + (0,),                         # the reference's defaults
    (0.45, 1.06, 0.18, 1.0, 0.1, 0, 0),      # DoTonemapAndSrgbTransform = 0 (the DoDebugBVHTraversal path): clamp, dither
    (-2.0, 1.06, 0.18, 1.0, 0.1, 1, 0),      # Exposure -2
    (3.0, 1.06, 0.18, 1.0, 0.1, 1, 0),       # Exposure +3
    (0.45, 0.0, 0.18, 1.0, 0.1, 1, 0),       # Saturation 0
    (0.45, 1.5, 0.18, 1.0, 0.1, 1, 0),       # Saturation 1.5
    (0.45, 1.06, 0.18, 1.0, 0.0, 1, 0),      # Compression 0.0
    (0.45, 1.06, 0.18, 1.0, 0.4, 1, 0),      # Compression 0.4
    (0.45, 1.06, 0.5, 0.8, 0.1, 1, 0),       # Peak 0.8 with Linear 0.5
    DEFAULTS + (1,),                         # the defaults with a bloom image added (Sampler1)
)

# Dither's BayerMatrix8 as the numerators k of its entries k / 65.0, in the shader's own row order: entry [i][j] is indexed [x % 8][y % 8]
BAYER = np.array([[1, 49, 13, 61, 4, 52, 16, 64], [33, 17, 45, 29, 36, 20, 48, 32], [9, 57, 5, 53, 12, 60, 8, 56], [41, 25, 37, 21, 44, 28, 40, 24],
                  [3, 51, 15, 63, 2, 50, 14, 62], [35, 19, 47, 31, 34, 18, 46, 30], [11, 59, 7, 55, 10, 58, 6, 54], [43, 27, 39, 23, 42, 26, 38, 22]], np.int32)


def _lcg(n, seed):
    """n values in [0, 1): multiples of 2^-16 from a 32-bit linear congruential sequence (the same on every platform)."""
    out = np.empty(n, np.float64); s = seed
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = (s >> 16) / 65536.0
    return out


def input_image():
    """(H, W, 4) float32, by formula.  Rows: 0-3 grey 0..2 (exact 0 at x = 0); 4-7 dense grey ramps across the DualSection joint Peak * Linear of every case (the joint sits at
    grey * 2^Exposure = Peak * Linear: 0.132, 0.293, 0.0225, 0.72); 8-11 dense grey ramps across the sRGB cutoff 0.0031308 of the cases (grey 0.0023, 0.0125, 0.00039) and a
    coloured one; 12-15 geometric ramps 1 .. 1e4, grey and coloured; 16-23 strongly saturated primaries and secondaries 0 .. 4; 24-27 negative components; 28-39 pseudo-random
    colours in [-0.25, 2.75).  Alpha is 1 (the shader reads .rgb).  No NaN, no Inf."""
    t = np.arange(W, dtype=np.float64) / (W - 1)
    img = np.zeros((H, W, 4), np.float64); img[..., 3] = 1.0
    grey = lambda a, b: (a + (b - a) * t)[:, None] * np.ones(3)
    img[0:4, :, :3] = grey(0.0, 2.0)
    img[4, :, :3] = grey(0.10, 0.16); img[5, :, :3] = grey(0.25, 0.33); img[6, :, :3] = grey(0.015, 0.03); img[7, :, :3] = grey(0.6, 0.85)
    img[8, :, :3] = grey(0.0015, 0.0035); img[9, :, :3] = grey(0.010, 0.015); img[10, :, :3] = grey(0.0003, 0.0005)
    img[11, :, :3] = (0.0005 + 0.006 * t)[:, None] * np.array([1.0, 0.5, 0.25])
    geo = 10.0 ** (4.0 * t)
    img[12, :, :3] = geo[:, None] * np.ones(3); img[13, :, :3] = geo[:, None] * np.array([1.0, 0.3, 0.05]); img[14, :, :3] = geo[:, None] * np.array([0.02, 0.6, 1.0]); img[15, :, :3] = geo[::-1, None] * np.array([0.4, 1.0, 0.1])
    for k, c in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 0.02, 0.02), (0.01, 0.01, 1))):
        img[16 + k, :, :3] = (4.0 * t * t)[:, None] * np.array(c, np.float64)
    img[24, :, :3] = np.stack([-0.5 + 1.5 * t, 0.3 + 0 * t, 0.8 - t], -1); img[25, :, :3] = np.stack([0.2 + 0 * t, -1.0 + 1.2 * t, t], -1)
    img[26, :, :3] = np.stack([t, 0.5 * t, -0.001 - t], -1); img[27, :, :3] = -grey(0.0, 3.0) + np.array([0.0, 0.5, 1.5])
    rnd = _lcg(12 * W * 3, 12345).reshape(12, W, 3)
    img[28:40, :, :3] = rnd * 3.0 - 0.25
    out = img.astype(np.float32)
    assert out[0, 0, 0] == 0.0 and (out[..., :3] < 0).any() and out.max() == np.float32(1e4) and np.isfinite(out).all()
    return out


def bloom_image():
    """(H, W, 4) float32: the second input of the bloom case (Sampler1): a smooth non-negative glow, strongest in the middle rows."""
    y = (np.arange(H, dtype=np.float64) / (H - 1))[:, None]; x = (np.arange(W, dtype=np.float64) / (W - 1))[None, :]
    g = 0.35 * np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) * 6.0)
    img = np.zeros((H, W, 4), np.float64); img[..., 0] = g; img[..., 1] = 0.8 * g; img[..., 2] = 0.5 * g + 0.01 * x; img[..., 3] = 1.0
    return img.astype(np.float32)


# ---- mat3, column-major like GLSL: m[c][r] --------------------------------------------------------------------------------------------------------------------------------
def _inverse(m):
    a = lambda r, c: m[c][r]
    det = a(0, 0) * (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(1, 2) * a(2, 0)) + a(0, 2) * (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0))
    inv = [[None] * 3 for _ in range(3)]                                  # inv[c][r]
    inv[0][0] = (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) / det; inv[1][0] = (a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2)) / det; inv[2][0] = (a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)) / det
    inv[0][1] = (a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2)) / det; inv[1][1] = (a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0)) / det; inv[2][1] = (a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)) / det
    inv[0][2] = (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)) / det; inv[1][2] = (a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1)) / det; inv[2][2] = (a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)) / det
    return inv


def _mul_mv(m, v):
    return [m[0][r] * v[0] + m[1][r] * v[1] + m[2][r] * v[2] for r in range(3)]


def _mul_mm(A, B):
    return [[A[0][r] * B[c][0] + A[1][r] * B[c][1] + A[2][r] * B[c][2] for r in range(3)] for c in range(3)]


def _unproject(xy, f):
    Y = f(1.0)
    return [(xy[0] * Y) / xy[1], Y, ((f(1.0) - xy[0] - xy[1]) * Y) / xy[1]]


def _primaries_to_matrix(r, g, b, w, f):
    R, G, B, Wh = _unproject(r, f), _unproject(g, f), _unproject(b, f), _unproject(w, f)
    temp = [[R[0], f(1.0), R[2]], [G[0], f(1.0), G[2]], [B[0], f(1.0), B[2]]]
    scale = _mul_mv(_inverse(temp), Wh)
    return [[R[i] * scale[0] for i in range(3)], [G[i] * scale[1] for i in range(3)], [B[i] * scale[2] for i in range(3)]]


def _mix(x, y, a, f):
    return x * (f(1.0) - a) + y * a


def matrices(settings, dtype=np.float32):
    """(sRGB_to_adjusted, inverse(sRGB_to_adjusted), pow(2, Exposure)) of AgX_DS: what depends on the settings alone.  Matrices as m[c][r] lists of `dtype` scalars."""
    f = dtype
    exposure, compression = f(np.float32(settings[0])), f(np.float32(settings[4]))
    xyR, xyG, xyB, xyW = [f(0.64), f(0.33)], [f(0.3), f(0.6)], [f(0.15), f(0.06)], [f(0.3127), f(0.3290)]
    srgb_to_xyz = _primaries_to_matrix(xyR, xyG, xyB, xyW, f)
    sf = f(1.0) / (f(1.0) - compression)
    Rc, Gc, Bc = [[_mix(xyW[i], p[i], sf, f) for i in range(2)] for p in (xyR, xyG, xyB)]
    adjusted_to_xyz = _primaries_to_matrix(Rc, Gc, Bc, xyW, f)
    m = _mul_mm(srgb_to_xyz, _inverse(adjusted_to_xyz))
    minv = _inverse(m)
    e2 = np.power(f(2.0), exposure)
    assert all(type(v) is f for col in m + minv for v in col) and type(e2) is f
    return m, minv, e2


def dither_values(dtype=np.float32):
    """(8, 8) of `dtype`, indexed [x % 8][y % 8]: (BayerMatrix8[x][y] - 0.5) / 64 with the entries k / 65.0."""
    f = dtype
    return ((BAYER.astype(f) / f(65.0) - f(0.5)) / f(64.0)).astype(f)


def present(img, settings, add0=None, add1=None, dtype=np.float32, first_row=0):
    """(H, W, 4) of `dtype`: vec4(ditherdColor, 1.0) for every texel of `img` ((H, W, 4) float32); add0 / add1 = Sampler1 / Sampler2 or None (+ 0.0).
    first_row: the image row of img's row 0 (the dither is indexed with rows of the whole frame)."""
    f = dtype
    sat, lin, peak = (f(np.float32(settings[k])) for k in (1, 2, 3))
    h, w = img.shape[:2]
    hdr = (np.zeros((h, w, 3), f) + img[..., :3].astype(f)) + (add0[..., :3].astype(f) if add0 is not None else f(0.0))
    hdr = hdr + (add1[..., :3].astype(f) if add1 is not None else f(0.0))
    if int(settings[5]):
        m, minv, e2 = matrices(settings, f)
        c = np.fmax(hdr, f(0.0)) * e2                                        # gmax: a NaN operand is dropped (fmaxf)
        c = np.stack(_mul_mv(m, [c[..., 0], c[..., 1], c[..., 2]]), -1)
        S = peak * lin
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            C = peak / (peak - S)
            upper = peak - (peak - S) * np.exp((-C * (c - S)) / peak)
        c = np.where(c < S, c, upper)
        c = np.fmin(np.fmax(c, f(0.0)), f(1.0))
        des = c[..., 0] * f(0.2126729) + c[..., 1] * f(0.7151522) + c[..., 2] * f(0.0721750)
        c = des[..., None] * (f(1.0) - sat) + c * sat
        c = np.fmin(np.fmax(c, f(0.0)), f(1.0))
        c = np.stack(_mul_mv(minv, [c[..., 0], c[..., 1], c[..., 2]]), -1)
        with np.errstate(invalid="ignore"):
            higher = f(1.055) * np.power(c, f(1.0) / f(2.4)) - f(0.055)
        c = np.where(c < f(0.0031308), c * f(12.92), higher)
    else:
        c = np.fmin(np.fmax(hdr, f(0.0)), f(1.0))
    d = dither_values(f)
    xs = np.arange(w) % 8; ys = (np.arange(h) + first_row) % 8
    c = c + d[xs[None, :], ys[:, None]][..., None]
    assert c.dtype == np.dtype(f)
    out = np.ones((h, w, 4), f); out[..., :3] = c
    return out


def quantise(x):
    """IDKPT_DISPLAY_RGBA8 of the RGBA32F display `x` ((.., 4) float32): the header's rule, in binary32; alpha 255."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    q = np.rint(np.fmin(np.fmax(x, np.float32(0.0)), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)   # fmaxf / fminf: no NaN reaches the integer conversion
    q[..., 3] = 255
    return q


def err(X, T):
    """max |X - T| over R, G, B (T: the binary64 evaluation); the output lives in [0, 1], so the error is absolute."""
    d = np.abs(np.asarray(X, np.float64)[..., :3] - np.asarray(T, np.float64)[..., :3])
    return float(d.max()) if np.isfinite(d).all() else float("inf")


def case_inputs(case):
    """(img, add0) of a case."""
    return input_image(), (bloom_image() if case[6] else None)


def load_fixture():
    """[(case tuple, llvmpipe's RGBA32F (H, W, 4) float32, llvmpipe's RGBA8 (H, W, 4) uint8)] of tests/golden/present/agx.npz, in the order of CASES; the inputs are
    checked against input_image() / bloom_image()."""
    fx = np.load(FIXTURE)
    assert fx["input"].tobytes() == input_image().tobytes() and fx["bloom"].tobytes() == bloom_image().tobytes()
    s = fx["settings"]; out = []
    for k in range(len(s)):
        case = tuple(float(np.float32(v)) for v in s[k]) + (int(fx["do_tonemap"][k]), int(fx["with_bloom"][k]))
        out.append((case, fx[f"float_{k}"], fx[f"bytes_{k}"]))
    return out
