"""The numpy restatement of idkptRectifyHistory, written from the contract in include/idkpt.h ("history rectification"), not from the C++: the mean disagreement of the
fast and the long history over the texels of the same surface in a (2R + 1)^2 window, its squared ratio to its own standard error, and the blend of the long history
towards the fast one.  Every operation a binary32 + - * / in the header's order; numpy's float32 array arithmetic rounds each operation correctly and fuses nothing,
np.fmax / np.fmin ignore a NaN operand as fmaxf / fminf do, so the result is the contract's bit for bit.  tests/test_rectify_ref.py holds the host build of
csrc/rectify_texel.hpp to it, tests/test_gpu_rectify.py the device."""
import os
import subprocess
import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(Radius=2, ZLow=3.0, ZHigh=6.0, Epsilon=1e-3)          # include/idkpt.h
FLT_MAX = F(3.402823466e+38)
BRANCH_FEW, BRANCH_ZERO, BRANCH_RAMP, BRANCH_FULL, BRANCH_NOT_FINITE = 0, 1, 2, 3, 4   # stats["branch"]: cnt < 4; lambda = 0 (or NaN); 0 < lambda < 1; lambda = 1; lambda > 0 and f_p or t_p not finite


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def nan_same(a, b):
    """bit for bit, except that a NaN equals a NaN (which NaN an operation on NaNs returns is not part of the contract)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def asfloat(u):
    return np.ascontiguousarray(u, np.uint32).view(F)


def _finite(a):
    return np.abs(a) <= FLT_MAX                    # false for NaN and for either infinity


def rectify(t, f, g, Radius=2, ZLow=3.0, ZHigh=6.0, Epsilon=1e-3, stats=None):
    """(H, W, 4) float32: the slot's temporal image after idkptRectifyHistory.  t, f: the temporal and the fast temporal image, g: the geometry image.
    stats (a dict) receives lambda (H, W; as computed, also where the pixel was left alone), cnt (H, W), branch (H, W; BRANCH_*) and blended (H, W bool)."""
    t = np.ascontiguousarray(t, F); f = np.ascontiguousarray(f, F); g = np.ascontiguousarray(g, F)
    H, W = t.shape[:2]
    R = int(Radius)
    assert 1 <= R <= 3 and t.shape == f.shape == g.shape == (H, W, 4)
    eps2 = F(Epsilon) * F(Epsilon); lo2 = F(ZLow) * F(ZLow); span = F(ZHigh) * F(ZHigh) - lo2
    ids = bits(g[..., 3])
    zero, one = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        d = f[..., :3] - t[..., :3]
        ok_d = _finite(d).all(axis=-1)
        cnt = np.zeros((H, W), F); s1 = np.zeros((H, W, 3), F); s2 = np.zeros((H, W, 3), F)
        ys, xs = np.mgrid[0:H, 0:W]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)      # (a clamped texel stands in where `inside` is false and is never used)
                ok = inside & (ids[cy, cx] == ids) & ok_d[cy, cx]
                dq = d[cy, cx]
                cnt = np.where(ok, cnt + one, cnt)
                s1 = np.where(ok[..., None], s1 + dq, s1)
                s2 = np.where(ok[..., None], s2 + dq * dq, s2)
        c = cnt[..., None]
        m = s1 / c
        var = np.fmax(s2 / c - m * m, zero)
        se2 = var / (c - one)
        z2c = (m * m) / (se2 + eps2)
        z2 = np.fmax(np.fmax(z2c[..., 0], z2c[..., 1]), z2c[..., 2])
        lam = np.fmin(np.fmax((z2 - lo2) / span, zero), one)
        few = cnt < F(4.0)
        own = _finite(f).all(axis=-1) & _finite(t).all(axis=-1)
        blended = ~few & (lam > zero) & own
        mixed = t + (f - t) * lam[..., None]
        out = np.where(blended[..., None], mixed, t).astype(F)
    if stats is not None:
        branch = np.full((H, W), BRANCH_ZERO, np.int32)
        branch[(lam > zero) & (lam < one)] = BRANCH_RAMP
        branch[lam == one] = BRANCH_FULL
        branch[(lam > zero) & ~own] = BRANCH_NOT_FINITE
        branch[few] = BRANCH_FEW
        stats.update({"lambda": lam, "cnt": cnt, "branch": branch, "blended": blended})
    return out


def rectify_moments(moments, out, blended):
    """the slot's temporal moments image after the call: .w = out.a where the blend branch ran, nothing else changes"""
    m = np.array(moments, F, copy=True)
    m[..., 3] = np.where(blended, out[..., 3], m[..., 3])
    return m


# ---- inputs both the host program and the device are held to
def random_images(W, H, seed, change=0.5, share=0.5):
    """(t, f, g): a long history t (counts 8 .. 32), a fast history f = t + noise (counts 1 .. 4), and — inside a random half-plane covering about `share` of the frame —
    a lighting change of `change` added to f, graded from 0 at the boundary, so that windows below, inside and above the ramp exist; ids in bands and a few lone pixels
    (cnt < 4), some missing ids"""
    rng = np.random.default_rng(seed)
    t = np.empty((H, W, 4), F); t[..., :3] = rng.random((H, W, 3)) * 2.0; t[..., 3] = rng.integers(8, 33, (H, W))
    noise = (rng.standard_normal((H, W, 3)) * 0.05).astype(F)
    ys, xs = np.mgrid[0:H, 0:W]
    a = rng.random() * 2.0 * np.pi
    side = (xs - W / 2.0) * np.cos(a) + (ys - H / 2.0) * np.sin(a) + (share - 0.5) * max(W, H)
    grade = np.clip(side / (0.35 * max(W, H, 2)), 0.0, 1.0)
    f = np.empty_like(t)
    f[..., :3] = t[..., :3] + noise + (change * grade)[..., None].astype(F) * F([1.0, 0.7, 0.4])
    f[..., 3] = rng.integers(1, 5, (H, W))
    ids = ((xs // 9 + 2 * (ys // 11)) % 5).astype(np.uint32)
    lone = rng.random((H, W)) < 0.04
    ids[lone] = (1000 + np.arange(int(lone.sum()))).astype(np.uint32)         # every lone pixel its own id: cnt = 1
    ids[rng.random((H, W)) < 0.02] = 0xFFFFFFFF                              # misses: an id like any other
    g = np.empty_like(t); g[..., :3] = rng.standard_normal((H, W, 3)); g[..., 3] = asfloat(ids)
    return t, f, g


PLANTS = [("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("flt_max", float(FLT_MAX)), ("-flt_max", -float(FLT_MAX)), ("subnormal", 1e-41), ("-subnormal", -1e-41)]


def planted(t, f, g, seed):
    """copies of (t, f) with NaN, +-Inf, +-FLT_MAX (the difference overflows where the other history has the other sign) and subnormals planted in f, in t and in either
    alpha, a few dozen texels each"""
    rng = np.random.default_rng(seed)
    t, f = t.copy(), f.copy()
    H, W = t.shape[:2]
    n = max(1, (H * W) // 40)
    for img in (f, t):
        for _, val in PLANTS:
            for ch in (0, 1, 2, 3):
                k = max(1, n // 8)
                img[rng.integers(0, H, k), rng.integers(0, W, k), ch] = F(val)
    # FLT_MAX against -FLT_MAX in the same texel: f - t overflows to +Inf although both are finite
    k = max(1, n // 4)
    y, x = rng.integers(0, H, k), rng.integers(0, W, k)
    f[y, x, 1] = FLT_MAX; t[y, x, 1] = -FLT_MAX
    return t, f, g


def uniform_change(W, H, seed, change=1.0):
    """every pixel of one surface, f = t + change exactly representable: var = 0 wherever the window is whole, lambda = 1 everywhere for a change far above Epsilon"""
    rng = np.random.default_rng(seed)
    t = np.empty((H, W, 4), F); t[..., :3] = rng.integers(0, 64, (H, W, 3)) * F(0.25); t[..., 3] = rng.integers(8, 33, (H, W))
    f = t.copy(); f[..., :3] = t[..., :3] + F(change); f[..., 3] = rng.integers(1, 5, (H, W))
    g = np.zeros_like(t); g[..., :3] = rng.standard_normal((H, W, 3)); g[..., 3] = asfloat(np.uint32([3]))[0]
    return t, f, g


# ---- the host build of the kernel's per-pixel function (tests/c_driver/rectify_host.cpp)
def build_host_program(exe, sanitize=True):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, "-Wall", "-Werror", os.path.join(HERE, "c_driver", "rectify_host.cpp"), "-o", exe])
    return exe


def host_rectify(exe, tmp, t, f, g, Radius=2, ZLow=3.0, ZHigh=6.0, Epsilon=1e-3):
    """(out (H, W, 4) float32, blended (H, W) bool): rectify_texel over a frame, the way k_rectify runs it"""
    H, W = t.shape[:2]
    src, dst = os.path.join(tmp, "rectify_in.bin"), os.path.join(tmp, "rectify_out.bin")
    with open(src, "wb") as fh:
        for part in (np.int32([W, H, Radius]), F([ZLow, ZHigh, Epsilon]), np.asarray(t, F), np.asarray(f, F), np.asarray(g, F)):
            fh.write(np.ascontiguousarray(part).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    raw = np.frombuffer(open(dst, "rb").read(), np.uint32)
    N = W * H
    assert raw.size == 5 * N
    return raw[:4 * N].view(F).reshape(H, W, 4).copy(), raw[4 * N:].reshape(H, W) != 0
