"""Variance-guided denoised output on the device: idkptDenoiseVariance (csrc/kernels_denoise_variance.hpp, the filter of include/idkpt.h "variance-guided denoised
output").  Everything is bit for bit: the filter against tests/denoise_variance_ref.py (the numpy restatement of the header's text), the result source against a context
that was given the same bytes through idkptUploadDenoised.  The 64 guard bytes behind the denoised image are looked at after every run.

Every context renders SAMPLES samples of the tiny Cornell box with the noise switch and OutputAOVs on, so that the accumulated count N is real; the planted cases then
overwrite Result, Albedo, Normal (idkptGetFrameDevicePtr) and the moments (idkptGetMomentsDevicePtr) through their device pointers with a torch copy on the context's
stream, as tests/test_gpu_denoise.py plants its images."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import denoise_ref as D  # noqa: E402
import denoise_variance_ref as R  # noqa: E402
from test_gpu_present import _stream, _alias, read_device, c_present, c_download  # noqa: E402
from test_gpu_denoise import write_frame, denoised_and_guard, c_denoise  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
NOISY, DENOISED = T.IDKPT_RESULT_NOISY, T.IDKPT_RESULT_DENOISED
RGBA8, RGBA32F = T.IDKPT_DISPLAY_RGBA8, T.IDKPT_DISPLAY_RGBA32F
ROUTE_NAMES = {T.IDKPT_DENOISE_ROUTE_TILED: "tiled", T.IDKPT_DENOISE_ROUTE_DIRECT: "direct"}


@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, variant="mixed")


def rendered(sc, w, h, samples=R.SAMPLES, noise=True, aovs=True, **kw):
    """a context that has accumulated `samples` samples of the box"""
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h, **kw)
    pt.UploadScene(sc); pt.SetCamera(S.cornell_camera(w, h)); pt.RayDepth = 3
    if aovs:
        pt.OutputAOVs = 1
    if noise:
        pt.SetNoiseEstimate(True)
    for _ in range(samples):
        pt.Compute()
    assert pt.AccumulatedSamples == samples
    return pt


def write_moments(pt, img, slot=None):
    import torch
    img = np.ascontiguousarray(img, np.float32)
    p, n = pt.moments_device_ptr(slot)
    assert n == img.nbytes
    st = _stream(pt)
    with torch.cuda.stream(st):
        _alias(p, n).copy_(torch.from_numpy(img.view(np.uint8).reshape(-1)).to("cuda"))
    st.synchronize()


def plant_images(pt, images, slot=0):
    for i, im in enumerate(images[:3]):
        write_frame(pt, im, i, slot)
    write_moments(pt, images[3], slot)


def c_variance(pt, s, slot=-1):
    d = s if isinstance(s, T.DenoiseVariance) else T.DenoiseVariance(**s)
    return pt._L.idkptDenoiseVariance(pt._ctx, slot, C.addressof(d))


def run_case(pt, s, slot=-1):
    pt._check(c_variance(pt, s, slot))
    body, guard = denoised_and_guard(pt, slot)
    assert (guard == 0xA5).all()
    return body


def differing(got, want):
    return int((R.bits(got) != R.bits(want)).any(axis=2).sum())


# ---- the filter, bit for bit
@pytest.mark.parametrize("case", range(len(R.CASES)), ids=[f"{w}x{h}-it{s['Iterations']}-demod{s['DemodulateAlbedo']}" for w, h, s in R.CASES])
def test_denoise_variance_equals_the_restatement_bit_for_bit(scene, case):
    W, H, s = R.CASES[case]
    pt = rendered(scene, W, H)
    images = R.random_images(W, H)
    plant_images(pt, images)
    got = run_case(pt, s)
    want = R.denoise_variance(*images, R.SAMPLES, **s)
    assert R.same(got, want), differing(got, want)
    # the route of every launch is the host code's rule, and the inputs are untouched
    assert [pt.denoise_route(i) for i in range(s["Iterations"])] == [R.route(i) for i in range(s["Iterations"])]
    for i in range(3):
        assert R.same(pt.FrameResult(0, i), images[i])
    assert R.same(pt.DownloadMoments(), images[3]) and pt.AccumulatedSamples == R.SAMPLES
    pt.Dispose()


def test_every_route_is_hit_by_the_cases():
    """tiled with spacing 1, 2 and 4 (k_denoise_var_tile<1 / 2 / 4>) and direct (k_denoise_var_direct, spacing 8 and up), on shapes with tile seams in both axes; the
    first launch as the last one (Iterations 1) and not; both values of the flag; variances at 0, clamped to 0 and large"""
    spacings = {(ROUTE_NAMES[R.route(i)], 1 << i) for W, H, s in R.CASES if (W, H) == (70, 41) for i in range(s["Iterations"])}
    assert {("tiled", 1), ("tiled", 2), ("tiled", 4), ("direct", 8), ("direct", 16), ("direct", 32)} <= spacings
    assert max(s["Iterations"] for _, _, s in R.CASES) == 8 and min(s["Iterations"] for _, _, s in R.CASES) == 1
    assert {(w, h) for w, h, _ in R.CASES} == set(R.SHAPES)
    for shape in ((1, 1), (5, 3), (16, 16), (37, 23), (70, 41)):
        assert {s["DemodulateAlbedo"] for w, h, s in R.CASES if (w, h) == shape} == {0, 1}
    images = R.random_images(37, 23)
    a = images[1][..., :3]
    assert (a == 0).any() and ((a > 0) & (a < R.EPS)).any()                     # albedo channels at 0 and below eps
    m1, m2 = images[3][..., 0], images[3][..., 1]
    v0 = R.variance_of_mean(images[3], R.SAMPLES)
    assert (m2 < m1 * m1).any() and (v0 == 0).any() and (v0 > 0.1).any() and np.isfinite(v0).all()


@pytest.mark.parametrize("plant", R.PLANTS, ids=[p[0] for p in R.PLANTS])
def test_non_finite_texels_stay_where_they_are(scene, plant):
    pname, which, channel = plant
    W, H = 37, 23
    clean = R.random_images(W, H)
    x, y = R.PLANT_POS
    mask = np.zeros((H, W), bool); mask[y, x] = True
    pt = rendered(scene, W, H)
    for name, value in R.NONFINITE:
        for s in R.PLANT_SETTINGS:
            images = R.plant(clean, which, value, R.PLANT_POS, channel)
            plant_images(pt, images)
            got = run_case(pt, s)
            want = R.denoise_variance(*images, R.SAMPLES, **s)
            assert R.same(got[~mask], want[~mask]), (name, s, differing(got, want))      # every other pixel equals the restatement
            assert R.same(got, want), (name, s)
            if which == 3 and name != "flt_max":
                skipped = R.denoise_variance(*clean, R.SAMPLES, skip=mask, **s)
                assert R.same(got[~mask], skipped[~mask]), (name, s)                     # a variance that is not finite: as if that position were outside the image
            elif which != 3:
                skipped = R.denoise_variance(*images, R.SAMPLES, tapskip=mask, **s)
                assert R.same(got[~mask], skipped[~mask]), (name, s)                     # a colour or guide: as if it were outside every other pixel's 25 taps
            if not s["DemodulateAlbedo"] and name != "flt_max":
                assert R.same(got[y, x, :3], images[0][y, x, :3])                         # the planted pixel stays what it was
    pt.Dispose()


# ---- a rendered frame, not planted
def test_a_rendered_frame_is_denoised_as_the_restatement_says_and_left_alone(scene):
    pt = rendered(scene, 48, 40, samples=3)
    images = [pt.FrameResult(0, i) for i in range(3)] + [pt.DownloadMoments()]
    assert np.abs(images[1][..., :3]).max() > 0 and np.abs(images[2][..., :3]).max() > 0 and images[3][..., 1].max() > 0      # guides and moments were accumulated
    got = pt.DenoiseVariance()
    want = R.denoise_variance(*images, 3, **R.DEFAULTS)
    assert R.same(got, want), differing(got, want)
    assert not R.same(got, images[0])
    _, guard = denoised_and_guard(pt)
    assert (guard == 0xA5).all()
    for i in range(3):
        assert R.same(pt.FrameResult(0, i), images[i])
    assert R.same(pt.DownloadMoments(), images[3]) and pt.AccumulatedSamples == 3
    pt.Dispose()


# ---- both filters fill the same image
def test_denoise_and_denoise_variance_each_leave_their_own_image(scene):
    W, H = 37, 23
    images = R.random_images(W, H)
    sv, sd = R.settings(4, 1), D.settings(4, 1)
    want_v, want_d = R.denoise_variance(*images, R.SAMPLES, **sv), D.denoise(*images[:3], **sd)
    assert not R.same(want_v, want_d)
    pt = rendered(scene, W, H)
    plant_images(pt, images)
    for _ in range(2):
        pt._check(c_denoise(pt, sd))
        body, guard = denoised_and_guard(pt)
        assert R.same(body, want_d) and (guard == 0xA5).all()
        assert R.same(run_case(pt, sv), want_v)
    pt._check(c_denoise(pt, sd))
    assert R.same(denoised_and_guard(pt)[0], want_d)
    pt.Dispose()


# ---- the result source
def test_present_shows_the_new_image_while_the_source_says_so(scene):
    W, H = 70, 41
    images = list(R.random_images(W, H)); images[0] = images[0].copy(); images[0][..., :3] *= 4.0
    s = R.settings(3, 1)
    tm = T.TonemapSettings()
    a, b = rendered(scene, W, H), rendered(scene, W, H)
    plant_images(a, images); plant_images(b, images)
    den = run_case(a, s)
    assert R.same(den, R.denoise_variance(*images, R.SAMPLES, **s))
    b.UploadDenoised(den)                                                        # the same bytes through idkptUploadDenoised
    for fmt in (RGBA8, RGBA32F):
        a._check(c_present(a, tm, fmt)); noisy = c_download(a, fmt)
        a.SetResultSource(DENOISED); b.SetResultSource(DENOISED)
        a._check(c_present(a, tm, fmt)); b._check(c_present(b, tm, fmt))
        assert R.same(c_download(a, fmt), c_download(b, fmt)) and not R.same(c_download(a, fmt), noisy)
        a.SetResultSource(NOISY); b.SetResultSource(NOISY)
    a.SetResultSource(DENOISED); b.SetResultSource(DENOISED)
    assert R.same(a.Bloom(None, 0), b.Bloom(None, 0))
    a.Dispose(); b.Dispose()


# ---- refusals: the status, and nothing launched
def test_refusals_leave_the_previous_image_as_it_was(scene):
    W, H = 16, 17
    images = R.random_images(W, H)
    good = R.settings(2, 1)
    pt = rendered(scene, W, H)
    plant_images(pt, images)
    before = run_case(pt, good)

    def unchanged():
        body, guard = denoised_and_guard(pt)
        return R.same(body, before) and (guard == 0xA5).all()

    nan, inf = float("nan"), float("inf")
    bad = [dict(good, Iterations=0), dict(good, Iterations=9), dict(good, LumaSigma=0.0), dict(good, LumaSigma=-1.0), dict(good, LumaSigma=nan), dict(good, LumaSigma=inf),
           dict(good, VarianceEpsilon=0.0), dict(good, VarianceEpsilon=-1e-3), dict(good, VarianceEpsilon=nan), dict(good, VarianceEpsilon=inf), dict(good, AlbedoSigma=inf),
           dict(good, AlbedoSigma=0.0), dict(good, NormalSigma=nan), dict(good, NormalSigma=-0.5), dict(good, DemodulateAlbedo=2), dict(good, DemodulateAlbedo=-1)]
    for s in bad:
        assert c_variance(pt, s) == INVALID_ARGUMENT and unchanged(), s
    d = T.DenoiseVariance(**good)
    for slot in (-2, 1):
        assert pt._L.idkptDenoiseVariance(pt._ctx, slot, C.addressof(d)) == INVALID_ARGUMENT
    assert pt._L.idkptDenoiseVariance(pt._ctx, -1, None) == INVALID_ARGUMENT and pt._L.idkptDenoiseVariance(None, -1, C.addressof(d)) == INVALID_ARGUMENT
    assert unchanged()
    # OutputAOVs = 0: the guides are not accumulated
    pt.OutputAOVs = 0
    assert c_variance(pt, good) == INVALID_OPERATION and unchanged()
    pt.OutputAOVs = 1
    assert c_variance(pt, good) == 0 and unchanged()                             # (the same call is accepted again: the refusals above were the ones named)
    # N < 2: straight after idkptResetAccumulation, and after one sample
    pt.ResetAccumulation()
    assert pt.AccumulatedSamples == 0 and c_variance(pt, good) == INVALID_OPERATION and unchanged()
    pt.Compute()
    assert pt.AccumulatedSamples == 1 and c_variance(pt, good) == INVALID_OPERATION and unchanged()
    # the switch off (turning it off restarts the accumulation; two samples later the count is not the reason)
    pt.SetNoiseEstimate(False)
    pt.Compute(); pt.Compute()
    assert pt.AccumulatedSamples == 2 and c_variance(pt, good) == INVALID_OPERATION and unchanged()
    pt._check(c_denoise(pt, D.settings(2, 1)))                                   # (idkptDenoise needs no switch)
    pt.Dispose()


def test_refusals_of_contexts_without_a_size_or_a_whole_frame(scene):
    W, H = 16, 17
    good = T.DenoiseVariance(**R.settings(2, 1))
    from idkengine_amd import _lib
    L = _lib.load()
    raw = C.c_void_p()
    assert L.idkptCreate(1, (C.c_int32 * 1)(0), C.byref(raw)) == 0
    assert L.idkptDenoiseVariance(raw, -1, C.addressof(good)) == INVALID_OPERATION                 # no size set
    assert L.idkptDestroy(raw) == 0
    # a row-band context and a two-member context: neither can turn the switch on, neither may run the filter; a denoised image there is none to keep
    bands = rendered(scene, W, H, samples=0, noise=False, row_modulo=2, row_remainder=1, row_band=8)
    group = rendered(scene, W, H, samples=0, noise=False, devices=[0, 0])
    buf = np.zeros((H, W, 4), np.float32)
    for pt in (bands, group):
        assert pt._L.idkptSetNoiseEstimate(pt._ctx, 1) == INVALID_OPERATION
        assert c_variance(pt, good) == INVALID_OPERATION
        assert pt._L.idkptDownloadDenoised(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
        pt.Dispose()
