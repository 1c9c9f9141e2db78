"""idkptDenoise on the CPU: tests/denoise_ref.py (the numpy binary32 restatement of the contract in include/idkpt.h) against hand-computed cases, against the properties a
denoiser has to have (noise falls, edges hold, non-finite texels stay where they are), and against the per-pixel function the device kernels call
(idkengine_amd/csrc/denoise_texel.hpp) compiled for the host under ASan/UBSan as a stand-alone program (tests/c_driver/denoise_host.cpp), bit for bit.

Two sentences of the issue are narrowed here to what its own contract (out = sum / sumW) gives:
 * "constant images: out = c exactly" holds through the division for constants whose products with h = m / 256 are exact; the test uses such constants (0.5, 0.75, 3.0).
 * "the planted pixel keeps its bits" holds for NaN and the infinities (every tap, the pixel's own included, is dropped: sumW == 0).  FLT_MAX in a GUIDE drops the
   neighbours only, the pixel keeps its own tap and becomes (c * h) / h with h = 9/64: its bits when c * 9 is exact, else its value to one rounding per iteration.  FLT_MAX in
   the COLOUR does the same to the planted channel: (FLT_MAX * 9/64) / (9/64) is one ulp below FLT_MAX.  The test asserts exactly those values, computed here by hand."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import denoise_ref as R  # noqa: E402

F = np.float32
HUGE = 1e18                                          # sigmas under which every range kernel is 1 / (1 + <= 3e-36) = 1 exactly for differences up to 1
FIXTURE = os.path.join(HERE, "golden", "denoise", "cornell64.npz")


def flat_guides(H, W):
    a = np.full((H, W, 4), 0.5, F); n = np.zeros((H, W, 4), F); n[..., 2] = 1.0
    return a, n


# ---- the feature exists
def test_the_library_declares_and_exports_the_denoise_entry_points():
    from idkengine_amd import _lib, gputypes as T
    names = ["idkptDenoise", "idkptUploadDenoised", "idkptDownloadDenoised", "idkptGetDenoisedDevicePtr", "idkptGetDenoiseRoute", "idkptSetResultSource", "idkptGetResultSource"]
    L = _lib.load()
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.idkptGetAbiVersion() >= 12
    d = T.Denoise()
    assert C.sizeof(T.Denoise) == 20 and (d.Iterations, d.ColorSigma, d.AlbedoSigma, d.NormalSigma, d.DemodulateAlbedo) == (5, 8.0, F(0.2), 0.5, 1)
    assert R.DEFAULTS == dict(Iterations=5, ColorSigma=8.0, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1)
    assert (T.IDKPT_RESULT_NOISY, T.IDKPT_RESULT_DENOISED, T.IDKPT_DENOISE_ROUTE_TILED, T.IDKPT_DENOISE_ROUTE_DIRECT) == (0, 1, 0, 1)
    # without a device the calls refuse a NULL context like every other entry point
    assert L.idkptDenoise(None, 0, None) == 2 and L.idkptSetResultSource(None, 1) == 2 and L.idkptUploadDenoised(None, 0, None, 0) == 2


def test_struct_layout_matches_the_header(tmp_path):
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idkpt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(idkpt_denoise), offsetof(idkpt_denoise, Iterations), '
                 'offsetof(idkpt_denoise, ColorSigma), offsetof(idkpt_denoise, AlbedoSigma), offsetof(idkpt_denoise, NormalSigma), offsetof(idkpt_denoise, DemodulateAlbedo), IDKPT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    from idkengine_amd import gputypes as T
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(T.Denoise), T.Denoise.Iterations.offset, T.Denoise.ColorSigma.offset, T.Denoise.AlbedoSigma.offset, T.Denoise.NormalSigma.offset, T.Denoise.DemodulateAlbedo.offset, 13]


# ---- the host build of the kernels' per-pixel function
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/denoise_host.cpp + csrc/denoise_texel.hpp under ASan and UBSan, as a stand-alone program"""
    exe = str(tmp_path_factory.mktemp("denoise_host") / "denoise_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           os.path.join(HERE, "c_driver", "denoise_host.cpp"), "-o", exe])
    return exe


def run_host_program(exe, tmp, images, s):
    H, W = images[0].shape[:2]
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([W, H, s["Iterations"], s["DemodulateAlbedo"]], np.int32).tobytes())
        f.write(np.array([s["ColorSigma"], s["AlbedoSigma"], s["NormalSigma"]], F).tobytes())
        for im in images:
            f.write(np.ascontiguousarray(im, F).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    return np.frombuffer(open(dst, "rb").read(), F).reshape(H, W, 4)


def test_host_build_of_the_kernels_pixel_function_equals_the_restatement_bit_for_bit(host_program, tmp_path):
    assert sorted({c[:2] for c in R.CASES}) == sorted(R.SHAPES)                  # every shape of the GPU list
    for W, H, s in R.CASES:
        images = R.random_images(W, H)
        assert R.same(run_host_program(host_program, str(tmp_path), images, s), R.denoise(*images, **s)), (W, H, s)
    clean = R.random_images(37, 23)
    for which in range(3):
        for name, value in R.NONFINITE:
            for s in R.PLANT_SETTINGS:
                images = R.plant(clean, which, value, R.PLANT_POS)
                assert R.same(run_host_program(host_program, str(tmp_path), images, s), R.denoise(*images, **s)), (which, name, s)


# ---- hand-computed cases
def test_a_single_pixel_is_returned_unchanged():
    c = np.array([[[0.3, 0.7, 1.1, 1.0]]], F); a, n = flat_guides(1, 1)
    for it in (1, 8):
        out = R.denoise(c, a, n, it, 1.0, 0.1, 0.25, 0)
        assert R.same(out, c)                  # (c * 9/64) / (9/64): one tap, h = 9/64, and these three products are exact to the bit after the division
    # with demodulation the pixel is (c / a) * a: exact for a = 0.5
    assert R.same(R.denoise(c, a, n, 3, 1.0, 0.1, 0.25, 1), c)


def test_constant_images_come_back_exactly_through_the_division():
    H, W = 6, 7
    c = np.ones((H, W, 4), F); c[..., :3] = np.array([0.5, 0.75, 3.0], F)           # products with h = m / 256 and their sums are exact
    a, n = flat_guides(H, W)
    for it in (1, 3):
        out = R.denoise(c, a, n, it, 0.37, 0.1, 0.25, 0)
        assert R.same(out, c)
    # the interior sums h to exactly 1, the edges to less: the division is what brings an edge pixel back
    acc = sum(R.K[dx + 2] * R.K[dy + 2] for dy in range(-2, 3) for dx in range(-2, 3))
    corner = sum(R.K[dx + 2] * R.K[dy + 2] for dy in range(0, 3) for dx in range(0, 3))
    assert acc == F(1.0) and corner == F(121.0 / 256.0)


def test_a_single_bright_texel_spreads_as_the_binomial_kernel():
    H = W = 9
    c = np.zeros((H, W, 4), F); c[..., 3] = 1.0; c[4, 4, :3] = 1.0
    a, n = flat_guides(H, W)
    out = R.denoise(c, a, n, 1, HUGE, HUGE, HUGE, 0)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16.0
    want = np.zeros((H, W), np.float64); want[2:7, 2:7] = np.outer(k, k)
    for ch in range(3):
        assert np.abs(out[..., ch].astype(np.float64) - want).max() <= 1e-6
    # every weight is h exactly (1 / (1 + 3e-36) = 1) and the pixels that see the texel have all 25 taps inside (sumW = 1): the binomial to the bit
    assert R.same(out[..., 0], want.astype(F)) and (out[..., 3] == 1.0).all()


def test_taps_outside_the_image_are_skipped_not_clamped():
    H = W = 5
    c = np.zeros((H, W, 4), F); c[..., 3] = 1.0; c[0, 0, :3] = 1.0
    a, n = flat_guides(H, W)
    out = R.denoise(c, a, n, 1, HUGE, HUGE, HUGE, 0)
    # the corner pixel: taps dx, dy in 0..2 only; h(0, 0) = 9/64 over sumW = (3/8 + 1/4 + 1/16)^2 = 121/256.  Clamped taps would repeat the bright texel 9 times.
    assert out[0, 0, 0] == F(9.0 / 64.0) / F(121.0 / 256.0) == F(36.0 / 121.0)
    # its right neighbour: dx in -1..2 (sum 15/16), dy in 0..2 (sum 11/16); the texel is its tap dx = -1, dy = 0: h = 1/4 * 3/8
    assert out[0, 1, 0] == F(3.0 / 32.0) / F(165.0 / 256.0)
    assert out[2, 2, 0] == F(1.0 / 256.0) and out[0, 3, 0] == 0.0 and out[3, 3, 0] == 0.0


# ---- noise falls
def test_noise_falls_on_a_flat_region(capsys):
    H = W = 64
    amp = F(0.1)
    rng = np.random.default_rng(7)
    c = np.ones((H, W, 4), F); c[..., :3] = F(0.5) + ((rng.random((H, W, 3)) * 2.0 - 1.0) * amp).astype(F)
    a, n = flat_guides(H, W)
    out = R.denoise(c, a, n, 1, 8.0 * float(amp), 0.1, 0.25, 0)
    rms = lambda im: float(np.sqrt(np.mean((im[2:-2, 2:-2, :3].astype(np.float64) - 0.5) ** 2)))
    factor = rms(out) / rms(c)
    with capsys.disabled():
        print(f"\n[denoise] flat 64 x 64, ColorSigma = 8 x amplitude, one iteration: RMS deviation x {factor:.4f} (unweighted filter: {70.0 / 256.0:.4f})")
    # the unweighted filter gives sqrt(sum h^2) = 70/256 = 0.273; the colour kernel only moves weight toward the centre
    assert factor <= 0.5


def test_the_tuned_defaults_lower_the_error_of_a_small_oracle_render(capsys):
    fx = np.load(FIXTURE)
    rmse = lambda x: float(np.sqrt(np.mean((x[..., :3].astype(np.float64) - fx["converged"][..., :3].astype(np.float64)) ** 2)))
    before, after = rmse(fx["result"]), rmse(R.denoise(fx["result"], fx["albedo"], fx["normal"], **R.DEFAULTS))
    with capsys.disabled():
        print(f"\n[denoise] 64 x 64 Cornell box, {int(fx['samples'][0])} against {int(fx['samples'][1])} samples: RMSE {before:.5f} -> {after:.5f} (x {after / before:.3f})")
    assert after < before


# ---- edges hold
@pytest.mark.parametrize("guide", ["albedo", "normal"])
def test_an_edge_in_a_guide_holds(guide):
    H, W, N = 16, 32, 4
    delta = F(0.5)
    c = np.ones((H, W, 4), F); c[..., :3] = np.array([0.2, 0.4, 0.6], F); c[:, W // 2:, :3] += delta
    a, n = flat_guides(H, W)
    sa, sn = 0.01, 0.25
    if guide == "albedo":
        a[:, W // 2:, 0] += F(100.0 * sa)                 # |d(a)| = 100 x AlbedoSigma across the edge
    else:
        n[:, W // 2:, :3] = np.array([0.0, 1.0, 0.0], F)  # |d(n)|^2 = 2 across the edge
        sn = float(np.sqrt(2.0)) / 100.0                  # ... = (100 x NormalSigma)^2
    out = R.denoise(c, a, n, N, 1.0, sa, sn, 0)
    bound = 2.0 * N * float(delta) / (1.0 + 100.0 ** 2)
    assert np.abs(out[..., :3].astype(np.float64) - c[..., :3].astype(np.float64)).max() <= bound
    # (and without the guide's step the edge does blur: the bound is not vacuous)
    a0, n0 = flat_guides(H, W)
    assert np.abs(R.denoise(c, a0, n0, N, 1.0, sa, 0.25, 0)[..., :3] - c[..., :3]).max() > 100 * bound


# ---- the non-finite rule
def own_tap_only(c, iterations):
    """(c * h) / h with h = 9/64, `iterations` times, in binary32"""
    h = F(9.0 / 64.0)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            c = (c * h) / h
    return c


@pytest.mark.parametrize("which", [0, 1, 2], ids=["colour", "albedo", "normal"])
@pytest.mark.parametrize("name,value", R.NONFINITE, ids=[n for n, _ in R.NONFINITE])
def test_a_non_finite_texel_stays_where_it_is(which, name, value):
    clean = R.random_images(37, 23)
    x, y = R.PLANT_POS
    mask = np.zeros((23, 37), bool); mask[y, x] = True
    others = ~mask
    for s in R.PLANT_SETTINGS:
        images = R.plant(clean, which, value, R.PLANT_POS)
        out = R.denoise(*images, **s)
        skipped = R.denoise(*clean, skip=mask, **s)
        # every other pixel: what it would be with taps at that position skipped
        assert R.same(out[others], skipped[others]), (s, int((R.bits(out) != R.bits(skipped)).any(axis=2).sum()))
        assert np.isfinite(out[others]).all()
        if s["DemodulateAlbedo"]:
            continue                                   # (the pixel's own value passes through (c / a) * a: covered by the comparison with the host build and the device)
        own = images[0][y, x, :3]
        if name != "flt_max":
            assert R.same(out[y, x, :3], own)           # every tap dropped, its own included: the bits stay
        else:
            want = own_tap_only(own.copy(), s["Iterations"])
            assert R.same(out[y, x, :3], want)
            if which == 0:
                assert R.bits(want[1]) == R.bits(np.finfo(F).max) - 1      # (FLT_MAX * 9/64) / (9/64): one ulp below, then stable
            assert np.abs(want.astype(np.float64) - own.astype(np.float64)).max() <= s["Iterations"] * float(np.abs(own.astype(np.float64)).max()) * 2.0 ** -23
