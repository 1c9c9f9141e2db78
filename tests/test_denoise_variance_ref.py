"""idkptDenoiseVariance on the CPU: tests/denoise_variance_ref.py (the numpy binary32 restatement of the contract in include/idkpt.h) against the properties the filter has
to have (the variance steers the edge, non-finite variances, colours and guides stay where they are), and against the per-pixel functions the device kernels call
(idkengine_amd/csrc/denoise_variance_texel.hpp) compiled for the host under ASan/UBSan as a stand-alone program (tests/c_driver/denoise_variance_host.cpp), bit for bit.

One sentence of the issue is narrowed here to what its own contract gives.  "Non-finite colour or guide: the same isolation as in test_denoise_ref.py" holds for the 25
taps — the weight of a tap at such a pixel is NaN or 0 — but the contract's prefilter skips a tap only when its VARIANCE is not finite, so the (finite) variance of a
pixel whose colour is not finite stays in its neighbours' g, and the pixel keeps (c, v) instead of being filtered.  The test therefore asserts: (1) on the planted input,
every other pixel is what it is with the position skipped in every other pixel's 25 taps (`tapskip`), and is finite; (2) after ONE iteration every other pixel equals the
CLEAN input's with that position skipped — the first prefilter reads v0, which the plant does not change (except a planted albedo under demodulation, whose v0 is divided
by another luminance: left to (1)); (3) the planted pixel keeps its colour's bits where every tap is dropped (NaN and the infinities, no demodulation)."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import denoise_variance_ref as R  # noqa: E402

F = np.float32


def flat_guides(H, W):
    a = np.full((H, W, 4), 0.5, F); n = np.zeros((H, W, 4), F); n[..., 2] = 1.0
    return a, n


# ---- the feature exists
def test_the_library_declares_and_exports_the_entry_point():
    from idkengine_amd import _lib, gputypes as T
    L = _lib.load()
    assert "idkptDenoiseVariance" in _lib.SYMBOLS and hasattr(L, "idkptDenoiseVariance")
    assert L.idkptGetAbiVersion() >= 12
    d = T.DenoiseVariance()
    assert C.sizeof(T.DenoiseVariance) == 24
    assert (d.Iterations, d.LumaSigma, d.VarianceEpsilon, d.AlbedoSigma, d.NormalSigma, d.DemodulateAlbedo) == (5, 1.0, F(0.1), F(0.2), 0.5, 1)
    assert R.DEFAULTS == dict(Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1)
    # without a device the call refuses a NULL context like every other entry point
    assert L.idkptDenoiseVariance(None, 0, None) == 2
    from idkengine_amd.pathtracer import PathTracer
    assert callable(PathTracer.DenoiseVariance)


def test_struct_layout_matches_the_header(tmp_path):
    fields = ["Iterations", "LumaSigma", "VarianceEpsilon", "AlbedoSigma", "NormalSigma", "DemodulateAlbedo"]
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idkpt.h"\nint main(void){printf("%zu ' + "%zu " * len(fields) + '%d\\n", sizeof(idkpt_denoise_variance), '
                 + ", ".join(f"offsetof(idkpt_denoise_variance, {f})" for f in fields) + ', IDKPT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    from idkengine_amd import gputypes as T
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(T.DenoiseVariance)] + [getattr(T.DenoiseVariance, f).offset for f in fields] + [13]
    assert got[:7] == [24, 0, 4, 8, 12, 16, 20]


# ---- the host build of the kernels' per-pixel functions
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/denoise_variance_host.cpp + csrc/denoise_variance_texel.hpp under ASan and UBSan, as a stand-alone program"""
    exe = str(tmp_path_factory.mktemp("denoise_variance_host") / "denoise_variance_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           os.path.join(HERE, "c_driver", "denoise_variance_host.cpp"), "-o", exe])
    return exe


def run_host_program(exe, tmp, images, N, s):
    H, W = images[0].shape[:2]
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([W, H, s["Iterations"], s["DemodulateAlbedo"], N], np.int32).tobytes())
        f.write(np.array([s["LumaSigma"], s["VarianceEpsilon"], s["AlbedoSigma"], s["NormalSigma"]], F).tobytes())
        for im in images:
            f.write(np.ascontiguousarray(im, F).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    return np.frombuffer(open(dst, "rb").read(), F).reshape(H, W, 4)


def test_host_build_of_the_kernels_pixel_functions_equals_the_restatement_bit_for_bit(host_program, tmp_path):
    assert sorted({c[:2] for c in R.CASES}) == sorted(R.SHAPES)                  # every shape of the GPU list
    for W, H, s in R.CASES:
        for N in (R.SAMPLES, 7):
            images = R.random_images(W, H, N=N)
            got, want = run_host_program(host_program, str(tmp_path), images, N, s), R.denoise_variance(*images, N, **s)
            assert R.same(got, want), (W, H, N, s, int((R.bits(got) != R.bits(want)).any(axis=2).sum()))
    clean = R.random_images(37, 23)
    for pname, which, channel in R.PLANTS:
        for name, value in R.NONFINITE:
            for s in R.PLANT_SETTINGS:
                images = R.plant(clean, which, value, R.PLANT_POS, channel)
                got, want = run_host_program(host_program, str(tmp_path), images, R.SAMPLES, s), R.denoise_variance(*images, R.SAMPLES, **s)
                assert R.same(got, want), (pname, name, s)


# ---- hand-computed cases
def test_the_variance_of_the_mean_and_its_demodulation():
    m = np.zeros((1, 4, 4), F)
    m[0, 0, :2] = (0.5, 0.75); m[0, 1, :2] = (0.5, 0.125); m[0, 2, :2] = (np.nan, 1.0); m[0, 3, :2] = (1.0, np.inf)
    v = R.variance_of_mean(m, 5)
    assert v[0, 0] == F(0.5) / F(4.0) and v[0, 1] == 0.0 and np.isposinf(v[0, 2]) and np.isposinf(v[0, 3])        # 0.75 - 0.25 = 0.5 over N - 1 = 4; the clamp; +Inf
    res = np.ones((1, 4, 4), F); alb = np.full((1, 4, 4), 0.5, F); alb[0, 1, :3] = 0.0                              # lum(floor(a)) = 0.5 (exact: the weights sum to 1), 1e-3-ish
    c0, v0 = R.first_state(res, alb, m, 5, 1)
    assert v0[0, 0] == F(0.125) / F(0.25) and (c0[0, 0] == 2.0).all() and v0[0, 1] == 0.0 and np.isposinf(v0[0, 2])
    c0, v0 = R.first_state(res, alb, m, 5, 0)
    assert v0[0, 0] == F(0.125) and (c0 == 1.0).all()


def test_a_single_pixel_is_returned_unchanged():
    c = np.array([[[0.3, 0.7, 1.1, 1.0]]], F); a, n = flat_guides(1, 1)
    m = np.array([[[0.7, 0.6, 0.0, 1.0]]], F)
    for it in (1, 8):
        out = R.denoise_variance(c, a, n, m, 3, it, 2.0, 1e-3, 0.1, 0.25, 0)
        assert R.same(out, c)                  # (c * 9/64) / (9/64): one tap, w = h / 1 = 9/64
    assert R.same(R.denoise_variance(c, a, n, m, 3, 3, 2.0, 1e-3, 0.1, 0.25, 1), c)       # (c / 0.5) * 0.5


def test_the_prefilter_is_the_binomial_over_the_taps_that_exist():
    v = np.zeros((5, 5), F); v[2, 2] = 16.0
    g = R.prefilter(v)
    want = np.zeros((5, 5), F); want[1:4, 1:4] = np.outer([1, 2, 1], [1, 2, 1]).astype(F)
    assert R.same(g, want)
    v[0, 0] = 16.0                             # the corner: taps ex, ey in 0 .. 1, sumG = (1/2 + 1/4)^2 = 9/16
    assert R.prefilter(v)[0, 0] == F(4.0) / F(9.0 / 16.0)    # its own tap alone is not 0: 16 / 4
    v[0, 1] = np.inf                           # not finite: skipped, sumG = 9/16 - 1/8
    assert R.prefilter(v)[0, 0] == F(4.0) / F(7.0 / 16.0)


def test_with_a_huge_variance_and_flat_guides_a_bright_texel_spreads_as_the_binomial_kernel():
    H = W = 9
    c = np.zeros((H, W, 3), F); c[4, 4] = 1.0
    a, n = flat_guides(H, W)
    v = np.full((H, W), 1e30, F)               # invL = 1 / (4e30 + eps): (dl * dl) * invL <= 3e-31, every den is 1 exactly
    out, vout = R.filter_state(c, v, a, n, 1, 2.0, 1e-3, 1.0, 1.0)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16.0
    want = np.zeros((H, W), np.float64); want[2:7, 2:7] = np.outer(k, k)
    assert R.same(out[..., 0], want.astype(F))
    # the variance of a weighted mean: sum h^2 v / (sum h)^2, in the interior (35/128)^2 v
    assert abs(float(vout[4, 4]) / 1e30 - (70.0 / 256.0) ** 2) < 1e-6


# ---- the variance steers the edge
def test_the_variance_steers_the_edge():
    H, W = 16, 32
    delta = F(0.25)
    c = np.full((H, W, 3), 0.5, F); c[:, W // 2:] += delta
    a, n = flat_guides(H, W)
    step = lambda im: float(im[:, W // 2, 0].astype(np.float64).mean() - im[:, W // 2 - 1, 0].astype(np.float64).mean())
    for it in (1, 3):
        converged, _ = R.filter_state(c, np.zeros((H, W), F), a, n, it, 4.0, 1e-4, 0.2, 0.5)
        noisy, _ = R.filter_state(c, np.full((H, W), 1.0, F), a, n, it, 4.0, 1e-4, 0.2, 0.5)
        # v0 = 0: invL = 1 / eps = 1e4, a tap across the step weighs h / (1 + 625); v0 = 1: invL = 1 / 16, h / (1 + 0.0039): the weight is monotone in g
        assert step(converged) > step(noisy) > 0.0, it
        assert step(converged) > 0.99 * float(delta) and step(noisy) < 0.6 * float(delta), (it, step(converged), step(noisy))


# ---- the non-finite rules
@pytest.mark.parametrize("channel", [0, 1], ids=["m1", "m2"])
@pytest.mark.parametrize("name,value", R.NONFINITE[:3], ids=[n for n, _ in R.NONFINITE[:3]])
def test_a_non_finite_variance_stays_where_it_is(channel, name, value):
    """NaN and the infinities in a moment make v0 = +Inf (FLT_MAX is a finite moment: a finite v0, covered by the comparison with the host build and the device)"""
    clean = R.random_images(37, 23)
    x, y = R.PLANT_POS
    mask = np.zeros((23, 37), bool); mask[y, x] = True
    others = ~mask
    for s in R.PLANT_SETTINGS:
        images = R.plant(clean, 3, value, R.PLANT_POS, channel)
        assert np.isposinf(R.first_state(images[0], images[1], images[3], R.SAMPLES, s["DemodulateAlbedo"])[1][y, x])
        out = R.denoise_variance(*images, R.SAMPLES, **s)
        skipped = R.denoise_variance(*clean, R.SAMPLES, skip=mask, **s)
        # every other pixel: what it would be with that position outside the image (25 taps and prefilter)
        assert R.same(out[others], skipped[others]), (s, int((R.bits(out) != R.bits(skipped)).any(axis=2).sum()))
        assert np.isfinite(out[others]).all()
        assert not R.same(out[others], R.denoise_variance(*clean, R.SAMPLES, **s)[others])       # (and the clean picture is another one)
        if not s["DemodulateAlbedo"]:
            assert R.same(out[y, x, :3], clean[0][y, x, :3])       # the pixel keeps its colour (through (c / a) * a otherwise)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["colour", "albedo", "normal"])
@pytest.mark.parametrize("name,value", R.NONFINITE, ids=[n for n, _ in R.NONFINITE])
def test_a_non_finite_colour_or_guide_stays_where_it_is(which, name, value):
    clean = R.random_images(37, 23)
    x, y = R.PLANT_POS
    mask = np.zeros((23, 37), bool); mask[y, x] = True
    others = ~mask
    for s in R.PLANT_SETTINGS:
        images = R.plant(clean, which, value, R.PLANT_POS)
        out = R.denoise_variance(*images, R.SAMPLES, **s)
        # (1) the planted input with the position skipped in every other pixel's 25 taps
        skipped = R.denoise_variance(*images, R.SAMPLES, tapskip=mask, **s)
        assert R.same(out[others], skipped[others]), (s, int((R.bits(out) != R.bits(skipped)).any(axis=2).sum()))
        assert np.isfinite(out[others]).all()
        # (2) one iteration: the clean input with the position skipped
        if not (which == 1 and s["DemodulateAlbedo"]):
            one = dict(s, Iterations=1)
            assert R.same(R.denoise_variance(*images, R.SAMPLES, **one)[others], R.denoise_variance(*clean, R.SAMPLES, tapskip=mask, **one)[others]), s
        # (3) every tap dropped, its own included: the bits stay
        if not s["DemodulateAlbedo"] and name != "flt_max":
            assert R.same(out[y, x, :3], images[0][y, x, :3])


# ---- the tuned defaults on a small render (measured, not a bound: asserted only to lower the error)
def test_the_tuned_defaults_lower_the_error_of_a_small_render_at_both_sample_counts(capsys):
    fx = np.load(os.path.join(HERE, "golden", "denoise", "cornell64_moments.npz"))
    conv = fx["converged"][..., :3].astype(np.float64)
    rmse = lambda x: float(np.sqrt(np.mean((x[..., :3].astype(np.float64) - conv) ** 2)))
    for n in (int(fx["samples"][0]), int(fx["samples"][1])):
        images = [fx[f"{name}{n}"] for name in ("result", "albedo", "normal", "moments")]
        before, after = rmse(images[0]), rmse(R.denoise_variance(*images, n, **R.DEFAULTS))
        with capsys.disabled():
            print(f"\n[denoise_variance] 64 x 64 Cornell box, {n} against {int(fx['samples'][2])} samples: RMSE {before:.5f} -> {after:.5f} (x {after / before:.3f})")
        assert after < before
