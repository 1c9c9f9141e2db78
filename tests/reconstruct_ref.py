"""The numpy restatement of idkptReconstructHistory, written from the contract in include/idkpt.h ("history reconstruction"), not from the C++: the pixels of a temporal
image whose count is below FillBelow gather colour, under the guide kernels and the taps' counts, from the texels of the same surface at p + Stride * (dx, dy) whose
count is at least FillBelow, and are topped up with it to at most FillBelow samples' worth.  Every operation a binary32 + - * / in the header's order; numpy's float32
array arithmetic rounds each operation correctly and fuses nothing, np.fmin ignores a NaN operand as fminf does, so the result is the contract's bit for bit.  The
restatement always reads the INPUT image and writes another one: that the device, which works in place, equals it is the in-place argument of the header put to the test.
tests/test_reconstruct_ref.py holds the host build of csrc/reconstruct_texel.hpp to it, tests/test_gpu_reconstruct.py the device."""
import os
import subprocess
import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(Radius=2, Stride=3, FillBelow=4.0, AlbedoSigma=0.2, NormalSigma=0.5)          # include/idkpt.h
FLT_MAX = F(3.402823466e+38)
MISS_ID = np.uint32(0xFFFFFFFF)
# stats["branch"]: rule 1 keeps the pixel; it walked its taps and S was not > 0; it blended; the blend was not finite
BRANCH_KEPT, BRANCH_NO_TAPS, BRANCH_WRITTEN, BRANCH_NOT_FINITE = 0, 1, 2, 3


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def asfloat(u):
    return np.ascontiguousarray(u, np.uint32).view(F)


def _finite(a):
    return np.abs(a) <= FLT_MAX                    # false for NaN and for either infinity


def _dist2(u, v):
    d = u - v
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def inv_sigma2(sigma):
    """1 / (sigma * sigma) in binary32 (ldexpf(sigma, 0) is sigma)"""
    s = F(sigma)
    return F(1.0) / (s * s)


def reconstruct(t, g, a, n, Radius=2, Stride=3, FillBelow=4.0, AlbedoSigma=0.2, NormalSigma=0.5, stats=None):
    """(H, W, 4) float32: the slot's temporal image after idkptReconstructHistory.  t: the temporal image, g: the geometry image, a, n: the accumulated Albedo and Normal
    images (H, W, >= 3).  stats (a dict) receives S (H, W), taps (H, W: the taps that contributed), branch (H, W; BRANCH_*) and written (H, W bool)."""
    t = np.ascontiguousarray(t, F); g = np.ascontiguousarray(g, F)
    a = np.ascontiguousarray(a, F)[..., :3]; n = np.ascontiguousarray(n, F)[..., :3]
    H, W = t.shape[:2]
    R, st = int(Radius), int(Stride)
    assert 1 <= R <= 3 and 1 <= st <= 8 and t.shape == g.shape == (H, W, 4) and a.shape == n.shape == (H, W, 3)
    fill = F(FillBelow)
    invA, invN = inv_sigma2(AlbedoSigma), inv_sigma2(NormalSigma)
    ids = bits(g[..., 3])
    zero, one = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        c = t[..., 3]
        ok_t = _finite(t).all(axis=-1)
        short = (ids != MISS_ID) & ok_t & (c < fill)                        # rule 1: the pixels that are filled
        donor = ok_t & (c >= fill)                                          # rule 2, the part that is the tap's own
        S = np.zeros((H, W), F); s = np.zeros((H, W, 3), F); taps = np.zeros((H, W), np.int32)
        ys, xs = np.mgrid[0:H, 0:W]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if dx == 0 and dy == 0:
                    continue
                qy, qx = ys + st * dy, xs + st * dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)      # (a clamped texel stands in where `inside` is false and is never used)
                w = one / ((one + _dist2(a[cy, cx], a) * invA) * (one + _dist2(n[cy, cx], n) * invN))
                ok = inside & (ids[cy, cx] == ids) & donor[cy, cx] & (w > zero)
                tq = t[cy, cx]
                k = w * tq[..., 3]
                S = np.where(ok, S + k, S)
                s = np.where(ok[..., None], s + tq[..., :3] * k[..., None], s)
                taps += ok
        b = np.fmin(S, fill - c)
        den = c + b
        rgb = (t[..., :3] * c[..., None] + (s / S[..., None]) * b[..., None]) / den[..., None]
        have = short & (S > zero)
        written = have & _finite(rgb).all(axis=-1)
        out = t.copy()
        out[..., :3] = np.where(written[..., None], rgb, t[..., :3])
    assert (bits(out[..., 3]) == bits(t[..., 3])).all()
    if stats is not None:
        branch = np.full((H, W), BRANCH_KEPT, np.int32)
        branch[short & ~have] = BRANCH_NO_TAPS
        branch[written] = BRANCH_WRITTEN
        branch[have & ~written] = BRANCH_NOT_FINITE
        stats.update({"S": np.where(short, S, zero), "taps": np.where(short, taps, 0), "branch": branch, "written": written, "short": short})
    return out


# ---- inputs both the host program and the device are held to
def random_images(W, H, seed, short_share=0.3):
    """(t, g, a, n): colours in 0 .. 2; counts 1 .. 3 on about `short_share` of the pixels (in blobs and as lone pixels), 4 .. 32 elsewhere, so that with FillBelow = 4 and
    with FillBelow = 8.5 both kinds exist; ids in bands, a few lone ids and misses; guides that vary smoothly with a few jumps"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    t = np.empty((H, W, 4), F); t[..., :3] = rng.random((H, W, 3)) * 2.0
    blob = (np.sin(xs * 0.9 + seed) + np.cos(ys * 0.7 - seed)) > 0.9
    short = blob | (rng.random((H, W)) < short_share * 0.5)
    t[..., 3] = np.where(short, rng.integers(1, 4, (H, W)), rng.integers(4, 33, (H, W)))
    ids = ((xs // 9 + 2 * (ys // 11)) % 5).astype(np.uint32)
    lone = rng.random((H, W)) < 0.03
    ids[lone] = (1000 + np.arange(int(lone.sum()))).astype(np.uint32)
    ids[rng.random((H, W)) < 0.03] = 0xFFFFFFFF
    g = np.empty_like(t); g[..., :3] = rng.standard_normal((H, W, 3)); g[..., 3] = asfloat(ids)
    a = np.ones((H, W, 4), F); n = np.ones((H, W, 4), F)
    a[..., :3] = (0.5 + 0.3 * np.sin(xs * 0.3)[..., None] + rng.random((H, W, 3)) * 0.1).astype(F)
    a[rng.random((H, W)) < 0.05, :3] = F(0.05)
    n[..., :3] = rng.standard_normal((H, W, 3)) * 0.2 + np.array([0.0, 0.0, 1.0])
    return t, g, a, n


PLANTS = [np.nan, np.inf, -np.inf, float(FLT_MAX), -float(FLT_MAX), 1e-41, -1e-41]


def planted(t, g, a, n, seed):
    """copies with NaN, +-Inf, +-FLT_MAX and subnormals planted in the colour, the count and both guides, and zero and negative counts, a few texels each"""
    rng = np.random.default_rng(seed)
    t, a, n = t.copy(), a.copy(), n.copy()
    H, W = t.shape[:2]
    k = max(1, (H * W) // 150)
    for img, chans in ((t, (0, 1, 2, 3)), (a, (0, 1, 2)), (n, (0, 1, 2))):
        for val in PLANTS:
            for ch in chans:
                img[rng.integers(0, H, k), rng.integers(0, W, k), ch] = F(val)
    for val in (0.0, -0.0, -1.0, -7.5):
        t[rng.integers(0, H, k), rng.integers(0, W, k), 3] = F(val)
    # a guide difference that overflows although both guides are finite: the weight is 0, the tap is dropped
    y, x = rng.integers(0, H, k), rng.integers(0, W, k)
    a[y, x, 1] = FLT_MAX; a[(y + 1) % H, x, 1] = -FLT_MAX
    return t, g, a, n


# ---- the host build of the kernel's per-pixel function (tests/c_driver/reconstruct_host.cpp)
def build_host_program(exe, sanitize=True):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, "-Wall", "-Werror", os.path.join(HERE, "c_driver", "reconstruct_host.cpp"), "-o", exe])
    return exe


def host_reconstruct(exe, tmp, t, g, a, n, Radius=2, Stride=3, FillBelow=4.0, AlbedoSigma=0.2, NormalSigma=0.5):
    """(out (H, W, 4) float32, written (H, W) bool): reconstruct_texel over a frame, reading the input image and writing another"""
    H, W = t.shape[:2]
    src, dst = os.path.join(tmp, "reconstruct_in.bin"), os.path.join(tmp, "reconstruct_out.bin")
    rgba = lambda im: np.ascontiguousarray(np.concatenate([np.asarray(im, F)[..., :3], np.ones((H, W, 1), F)], axis=2))   # noqa: E731
    with open(src, "wb") as fh:
        for part in (np.int32([W, H, Radius, Stride]), F([FillBelow, AlbedoSigma, NormalSigma]), np.asarray(t, F), np.asarray(g, F), rgba(a), rgba(n)):
            fh.write(np.ascontiguousarray(part).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    raw = np.frombuffer(open(dst, "rb").read(), np.uint32)
    N = W * H
    assert raw.size == 5 * N
    return raw[:4 * N].view(F).reshape(H, W, 4).copy(), raw[4 * N:].reshape(H, W) != 0
