"""The numpy restatement of idkptReprojectMoments and idkptDenoiseTemporal, written from the contract in include/idkpt.h ("temporal moments"), not from the C++: the
luminance moments blended through idkptReproject's taps, the per-pixel variance of the mean from them (each pixel's own effective sample count; a 7 x 7 guide-weighted
spatial estimate below SpatialBelow), and idkptDenoiseVariance's iterations on the temporal image.  Every operation a binary32 + - * / in the header's order; numpy's
float32 array arithmetic rounds each operation correctly and fuses nothing, so the result is the contract's bit for bit.  The tap geometry is tests/reproject_ref.py's
and the iterations are tests/denoise_variance_ref.py's: both are pinned by their own tests.  tests/test_denoise_temporal_ref.py holds the host build of
csrc/denoise_temporal_texel.hpp and csrc/reproject_texel.hpp to it, tests/test_gpu_denoise_temporal.py the device."""
import os
import subprocess
import numpy as np
import reproject_ref as P
import denoise_variance_ref as V

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1, SpatialBelow=4.0)   # include/idkpt.h
RADIUS = 3
bits, same, route = V.bits, V.same, V.route


# ---- idkptReprojectMoments
def start_moments(moments, n):
    """historySlot == IDKPT_NO_HISTORY: (m1, m2, 0, n)"""
    m = np.asarray(moments, F)
    out = np.zeros(m.shape[:2] + (4,), F)
    out[..., 0] = m[..., 0]; out[..., 1] = m[..., 1]; out[..., 3] = F(n)
    return out


def reproject_moments(moments, n, g, hg, hm, prev_proj_view, prev_view_pos, PositionTolerance=0.02, MaxHistory=32.0, stats=None):
    """(H, W, 4) float32: the temporal moments image.  moments: the slot's (m1, m2, 0, 1) image; g, hg: geometry images; hm: the history slot's temporal moments.
    The clip coordinates, taps, validity rules (all four channels of hm finite) and the blend are idkptReproject's with cur = (m1, m2); the third channel is stored as 0."""
    cur = start_moments(moments, 0)                # (the alpha of `cur` is not read)
    out = P.reproject(cur, n, g, hg, hm, prev_proj_view, prev_view_pos, PositionTolerance, MaxHistory, stats)
    out[..., 2] = F(0.0)
    return out


# ---- idkptDenoiseTemporal
def spatial_variance(tm, albedo, normal, invA, invN):
    """(v (H, W), sW (H, W)): the spatial estimate at EVERY pixel (the caller selects): 7 x 7 taps, dy the outer loop, dx the inner one"""
    tm = np.asarray(tm, F)
    a = np.ascontiguousarray(np.asarray(albedo, F)[..., :3]); n = np.ascontiguousarray(np.asarray(normal, F)[..., :3])
    M1, M2, cnt = tm[..., 0], tm[..., 1], tm[..., 3]
    H, W = M1.shape
    one = F(1.0)
    fin = np.isfinite(M1) & np.isfinite(M2)
    sM1 = np.zeros((H, W), F); sM2 = np.zeros((H, W), F); sW = np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                win = V._windows(H, W, 1, dx, dy)
                if win is None:
                    continue
                Pp, Q = win
                w = one / ((one + V._dist2(a, Pp, Q) * invA) * (one + V._dist2(n, Pp, Q) * invN))
                ok = (w > 0) & fin[Q]
                sM1[Pp] = np.where(ok, sM1[Pp] + M1[Q] * w, sM1[Pp])
                sM2[Pp] = np.where(ok, sM2[Pp] + M2[Q] * w, sM2[Pp])
                sW[Pp] = np.where(ok, sW[Pp] + w, sW[Pp])
        a1 = sM1 / sW; a2 = sM2 / sW
        v = np.fmax(a2 - a1 * a1, F(0.0)) / cnt
    return np.where(sW == 0, F(np.inf), v).astype(F), sW


def first_state(temporal, tm, albedo, normal, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1, SpatialBelow=4.0, branch=None):
    """(c0 (H, W, 3), v0 (H, W)) as the first iteration reads them.  `branch` (a dict, optional) receives the masks "nonfinite", "temporal", "spatial" and "sW" """
    c = np.ascontiguousarray(np.asarray(temporal, F)[..., :3]); a = np.asarray(albedo, F)[..., :3]
    tm = np.asarray(tm, F)
    M1, M2, cnt = tm[..., 0], tm[..., 1], tm[..., 3]
    invA, invN = V.inv_sigma2(AlbedoSigma), V.inv_sigma2(NormalSigma)
    bad = ~(np.isfinite(M1) & np.isfinite(M2) & np.isfinite(cnt))
    with np.errstate(all="ignore"):
        long = ~bad & (cnt >= F(SpatialBelow))
        vt = np.fmax(M2 - M1 * M1, F(0.0)) / (cnt - F(1.0))
        vs, sW = spatial_variance(tm, albedo, normal, invA, invN)
        v = np.where(bad, F(np.inf), np.where(long, vt, vs)).astype(F)
        if DemodulateAlbedo:
            fa = V.floor_albedo(a)
            c = (c / fa).astype(F)
            la = V.lum(fa)
            v = (v / (la * la)).astype(F)
    if branch is not None:
        branch.update(nonfinite=bad, temporal=long, spatial=~bad & ~long, sW=sW)
    return c, v


def denoise_temporal(temporal, tm, albedo, normal, Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1, SpatialBelow=4.0):
    """(H, W, 4) float32: rgb as the contract defines it, alpha 1.0.  temporal: the temporal image (its alpha is not read); tm: the temporal moments (M1, M2, 0, cnt)"""
    c, v = first_state(temporal, tm, albedo, normal, AlbedoSigma, NormalSigma, DemodulateAlbedo, SpatialBelow)
    c, v = V.filter_state(c, v, albedo, normal, Iterations, LumaSigma, VarianceEpsilon, AlbedoSigma, NormalSigma)
    with np.errstate(all="ignore"):
        if DemodulateAlbedo:
            c = (c * V.floor_albedo(np.asarray(albedo, F)[..., :3])).astype(F)
    out = np.ones(c.shape[:2] + (4,), F)
    out[..., :3] = c
    return out


# ---- the inputs both test files share (seeded; nothing here depends on the code under test)
SHAPES = [(1, 1), (3, 5), (16, 16), (17, 16), (37, 29), (64, 48)]      # (W, H): two smaller than the 7 x 7 window, one tile, a one-pixel spill, ragged, several tiles
COUNTS = np.array([1.0, 1.0, 1.0, 2.0, 3.0, 3.75, 4.0, 5.0, 7.25, 12.0, 33.0], F)   # effective sample counts on both sides of SpatialBelow = 4, 4 itself (>=: temporal) included


def settings(Iterations, DemodulateAlbedo, SpatialBelow=4.0, LumaSigma=2.0, VarianceEpsilon=1e-3, AlbedoSigma=0.2, NormalSigma=0.5):
    return dict(Iterations=Iterations, LumaSigma=LumaSigma, VarianceEpsilon=VarianceEpsilon, AlbedoSigma=AlbedoSigma, NormalSigma=NormalSigma, DemodulateAlbedo=DemodulateAlbedo,
                SpatialBelow=SpatialBelow)


# every shape with 1, 2 and 5 iterations (5 reaches the DIRECT route at spacings 8 and 16) and both values of the flag
CASES = [(W, H, settings(it, demod)) for W, H in SHAPES for it in (1, 2, 5) for demod in (0, 1)]


def random_images(W, H, seed=0):
    """(temporal, temporal moments, Albedo, Normal), (H, W, 4) float32 each: tests/denoise_variance_ref.py's synthetic frame (albedo channels at 0 and below eps, variances
    from 0 — clamped in places — to fireflies) with a per-pixel effective sample count drawn from COUNTS in the alpha of the first two"""
    result, albedo, normal, moments = V.random_images(W, H, seed, N=4)
    rng = np.random.default_rng(7000 * seed + 13 * W + H)
    cnt = COUNTS[rng.integers(0, len(COUNTS), (H, W))]
    temporal = result.copy(); temporal[..., 3] = cnt
    tm = moments.copy(); tm[..., 2] = 0.0; tm[..., 3] = cnt
    return temporal, tm, albedo, normal


NAN, INF = F(np.nan), F(np.inf)
NONFINITE = [("nan", NAN), ("+inf", INF), ("-inf", F(-np.inf))]
TEMPORAL, MOMENTS, ALBEDO, NORMAL = 0, 1, 2, 3
# (name, [(image, channel, value), ...]): what is written at the planted pixel
PLANTS = ([(f"{ch}={name}", [(MOMENTS, k, value)]) for ch, k in (("M1", 0), ("M2", 1), ("cnt", 3)) for name, value in NONFINITE]
          + [("cnt=0", [(MOMENTS, 3, F(0.0))])]
          + [(f"{gname}=nan at a spatial pixel", [(g, 1, NAN), (MOMENTS, 3, F(1.0))]) for gname, g in (("albedo", ALBEDO), ("normal", NORMAL))]     # every weight is NaN: sW == 0
          + [(f"rgb={name}", [(TEMPORAL, 1, value)]) for name, value in NONFINITE])
PLANT_SHAPE = (37, 29)
PLANT_POSITIONS = [(18, 11), (36, 28)]                 # (x, y): the interior (not on a tile seam's first column) and the corner of a partial tile
PLANT_SETTINGS = [settings(4, 0), settings(4, 1)]      # spacing 1, 2, 4 (tiled) and 8 (direct)


def plant(images, writes, pos):
    out = [im.copy() for im in images]
    for which, channel, value in writes:
        out[which][pos[1], pos[0], channel] = value
    return tuple(out)


# ---- the host build (tests/c_driver/denoise_temporal_host.cpp)
def build_host_program(exe, sanitize=True):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, "-Wall", "-Werror", os.path.join(HERE, "c_driver", "denoise_temporal_host.cpp"), "-o", exe])
    return exe


def _run(exe, mode, tmp, payload, shape):
    src, dst = os.path.join(tmp, f"{mode}_in.bin"), os.path.join(tmp, f"{mode}_out.bin")
    with open(src, "wb") as f:
        for part in payload:
            f.write(np.ascontiguousarray(part).tobytes())
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    return np.frombuffer(open(dst, "rb").read(), F).reshape(shape)


def host_filter(exe, tmp, images, s):
    H, W = images[0].shape[:2]
    return _run(exe, "filter", tmp, [np.int32([W, H, s["Iterations"], s["DemodulateAlbedo"]]), F([s["LumaSigma"], s["VarianceEpsilon"], s["AlbedoSigma"], s["NormalSigma"], s["SpatialBelow"]])]
                + [np.asarray(im, F) for im in images], (H, W, 4))


def host_moments(exe, tmp, moments, n, g, hg, hm, M, vp, PositionTolerance=0.02, MaxHistory=32.0, start=False):
    H, W = moments.shape[:2]
    return _run(exe, "moments", tmp, [np.int32([W, H, int(start)]), F([n]), np.asarray(M, F).reshape(16), np.asarray(vp, F).reshape(3), F([PositionTolerance, MaxHistory]),
                                      np.asarray(moments, F), np.asarray(g, F), np.asarray(hg, F), np.asarray(hm, F)], (H, W, 4))
