"""Denoised output on the device: idkptDenoise (csrc/kernels_denoise.hpp, the edge-avoiding a-trous filter of include/idkpt.h), idkptUploadDenoised,
idkptDownloadDenoised, idkptGetDenoisedDevicePtr, idkptGetDenoiseRoute and the result source (idkptSetResultSource) of idkptPresent and idkptBloom.  Everything is bit for
bit: the filter against tests/denoise_ref.py (the numpy restatement of the header's text), the result source against a second context that holds the same image as its
image 0.  The 64 guard bytes behind every denoised image are looked at after every run.

Chosen images are written through the device pointers (idkptGetFrameDevicePtr) and a torch copy on the context's stream, as tests/test_gpu_present.py plants its image."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import denoise_ref as R  # noqa: E402
from test_gpu_present import _stream, _alias, read_device, c_present, c_download  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
NOISY, DENOISED = T.IDKPT_RESULT_NOISY, T.IDKPT_RESULT_DENOISED
RGBA8, RGBA32F = T.IDKPT_DISPLAY_RGBA8, T.IDKPT_DISPLAY_RGBA32F
GUARD = 64
ROUTE_NAMES = {T.IDKPT_DENOISE_ROUTE_TILED: "tiled", T.IDKPT_DENOISE_ROUTE_DIRECT: "direct"}


def new_pt(w, h, aovs=True, **kw):
    """A context with a size and no scene: the denoise calls need nothing else (OutputAOVs is a setting)."""
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h, **kw)
    if aovs:
        pt.OutputAOVs = 1
    return pt


def write_frame(pt, img, image, slot=0):
    import torch
    img = np.ascontiguousarray(img, np.float32)
    p, n = pt.frame_device_ptr(slot, image)
    assert n == img.nbytes
    st = _stream(pt)
    with torch.cuda.stream(st):
        _alias(p, n).copy_(torch.from_numpy(img.view(np.uint8).reshape(-1)).to("cuda"))
    st.synchronize()


def plant_images(pt, images, slot=0):
    for i, im in enumerate(images):
        write_frame(pt, im, i, slot)


def c_denoise(pt, s, slot=-1):
    d = s if isinstance(s, T.Denoise) else T.Denoise(**s)
    return pt._L.idkptDenoise(pt._ctx, slot, C.addressof(d))


def denoised_and_guard(pt, slot=-1):
    """(the denoised image through the device pointer, its guard bytes); the download must agree"""
    p, n = pt.denoised_device_ptr(None if slot < 0 else slot)
    assert n == pt.height * pt.width * 16
    raw = read_device(pt, p, n + GUARD)
    body = raw[:n].view(np.float32).reshape(pt.height, pt.width, 4)
    assert R.same(body, pt.DownloadDenoised(None if slot < 0 else slot))       # the device pointer equals the download
    return body, raw[n:]


def run_case(pt, images, s, slot=-1):
    pt._check(c_denoise(pt, s, slot))
    body, guard = denoised_and_guard(pt, slot)
    assert (guard == 0xA5).all()
    return body


# ---- the filter, bit for bit
@pytest.mark.parametrize("case", range(len(R.CASES)), ids=[f"{w}x{h}-it{s['Iterations']}-demod{s['DemodulateAlbedo']}" for w, h, s in R.CASES])
def test_denoise_equals_the_restatement_bit_for_bit(case):
    W, H, s = R.CASES[case]
    pt = new_pt(W, H)
    images = R.random_images(W, H)
    plant_images(pt, images)
    got = run_case(pt, images, s)
    want = R.denoise(*images, **s)
    assert R.same(got, want), int((R.bits(got) != R.bits(want)).any(axis=2).sum())
    # the route of every launch is the host code's rule, and the inputs are untouched
    routes = [pt.denoise_route(i) for i in range(s["Iterations"])]
    assert routes == [R.route(i) for i in range(s["Iterations"])]
    for i, im in enumerate(images):
        assert R.same(pt.FrameResult(0, i), im)
    pt.Dispose()


def test_every_route_is_hit_by_the_cases():
    """tiled with spacing 1, 2 and 4 (k_denoise_tile<1 / 2 / 4>) and direct (k_denoise_direct, spacing 8 and up), on shapes with tile seams in both axes"""
    spacings = {(ROUTE_NAMES[R.route(i)], 1 << i) for W, H, s in R.CASES if (W, H) == (70, 41) for i in range(s["Iterations"])}
    assert {("tiled", 1), ("tiled", 2), ("tiled", 4), ("direct", 8), ("direct", 16), ("direct", 32)} <= spacings
    assert max(s["Iterations"] for _, _, s in R.CASES) == 8 and min(s["Iterations"] for _, _, s in R.CASES) == 1
    assert {s["DemodulateAlbedo"] for _, _, s in R.CASES} == {0, 1}
    a = R.random_images(37, 23)[1][..., :3]
    assert (a == 0).any() and ((a > 0) & (a < R.EPS)).any()                     # albedo channels at 0 and below eps


@pytest.mark.parametrize("which", [0, 1, 2], ids=["colour", "albedo", "normal"])
def test_non_finite_texels_stay_where_they_are(which):
    W, H = 37, 23
    clean = R.random_images(W, H)
    x, y = R.PLANT_POS
    mask = np.zeros((H, W), bool); mask[y, x] = True
    pt = new_pt(W, H)
    for name, value in R.NONFINITE:
        for s in R.PLANT_SETTINGS:
            images = R.plant(clean, which, value, R.PLANT_POS)
            plant_images(pt, images)
            got = run_case(pt, images, s)
            assert R.same(got, R.denoise(*images, **s)), (name, s)
            skipped = R.denoise(*clean, skip=mask, **s)
            assert R.same(got[~mask], skipped[~mask]), (name, s)               # every other pixel: as if taps at that position were outside
            if not s["DemodulateAlbedo"] and name != "flt_max":
                assert R.same(got[y, x, :3], images[0][y, x, :3])               # the planted pixel keeps its bits
    pt.Dispose()


# ---- a rendered frame
@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, variant="mixed")


def rendered(sc, samples, w=48, h=40):
    pt = new_pt(w, h)
    pt.UploadScene(sc); pt.SetCamera(S.cornell_camera(w, h)); pt.RayDepth = 3
    for _ in range(samples):
        pt.Compute()
    return pt


def test_a_rendered_frame_is_denoised_as_the_restatement_says_and_left_alone(scene):
    pt = rendered(scene, 3)
    images = [pt.FrameResult(0, i) for i in range(3)]
    assert np.abs(images[1][..., :3]).max() > 0 and np.abs(images[2][..., :3]).max() > 0      # the guides were accumulated
    got = pt.Denoise()
    assert R.same(got, R.denoise(*images, **R.DEFAULTS))
    _, guard = denoised_and_guard(pt)
    assert (guard == 0xA5).all()
    for i in range(3):
        assert R.same(pt.FrameResult(0, i), images[i])
    assert pt.AccumulatedSamples == 3
    for _ in range(2):
        pt.Compute()
    never = rendered(scene, 5)
    for i in range(3):
        assert R.same(pt.FrameResult(0, i), never.FrameResult(0, i))
    assert pt.AccumulatedSamples == never.AccumulatedSamples == 5
    pt.Dispose(); never.Dispose()


# ---- the result source
def chain_of(pt, bloom, slot=None):
    out = [pt.Bloom(bloom, 0, slot)]
    levels, _, _ = pt.bloom_info(slot)
    return out + [pt.bloom_level(0, l, slot) for l in range(levels)] + [pt.bloom_level(1, l, slot) for l in range(levels - 1)]


@pytest.mark.parametrize("pres", [None, (96, 54), (35, 20)], ids=["equal", "larger", "smaller"])
def test_present_and_bloom_read_the_denoised_image_while_the_source_says_so(pres):
    W, H = 70, 41
    images = R.random_images(W, H); images[0][..., :3] *= 40.0                    # (most of it above bloom's threshold)
    s = R.settings(3, 1)
    tm, bloom = T.TonemapSettings(), T.BloomSettings(MinusLods=1)
    a, b, never = new_pt(W, H), new_pt(W, H), new_pt(W, H)
    for pt in (a, b, never):
        if pres:
            pt.SetPresentationSize(*pres)
        plant_images(pt, images)
    den = run_case(a, images, s)
    write_frame(b, den, 0)                                                       # the second context holds the denoised image as its image 0, source NOISY
    shape = dict(rows=pres[1], width=pres[0]) if pres else {}
    # source NOISY after a denoise: as a context that never denoised
    for fmt in (RGBA8, RGBA32F):
        a._check(c_present(a, tm, fmt)); never._check(c_present(never, tm, fmt))
        assert R.same(c_download(a, fmt, **shape), c_download(never, fmt, **shape))
    assert all(R.same(x, y) for x, y in zip(chain_of(a, bloom), chain_of(never, bloom)))
    # source DENOISED: as the context whose image 0 is the denoised image
    a.SetResultSource(DENOISED)
    assert a.GetResultSource() == DENOISED and b.GetResultSource() == NOISY
    for fmt in (RGBA8, RGBA32F):
        a._check(c_present(a, tm, fmt)); b._check(c_present(b, tm, fmt))
        assert R.same(c_download(a, fmt, **shape), c_download(b, fmt, **shape))
    ca, cb = chain_of(a, bloom), chain_of(b, bloom)
    assert len(ca) == len(cb) and all(R.same(x, y) for x, y in zip(ca, cb)) and ca[0][..., :3].max() > 0
    assert not R.same(ca[0], chain_of(never, bloom)[0])                          # (and that is not the noisy picture)
    # images 1 and 2 ignore the source
    for image in (1, 2):
        a._check(c_present(a, tm, RGBA32F, image=image)); never._check(c_present(never, tm, RGBA32F, image=image))
        assert R.same(c_download(a, RGBA32F, **shape), c_download(never, RGBA32F, **shape))
        assert R.same(a.Bloom(bloom, image), never.Bloom(bloom, image))
    # image 3 is still refused, and the accumulated image is still what the downloads return
    assert c_present(a, tm, RGBA8, image=3) == INVALID_ARGUMENT and a._L.idkptBloom(a._ctx, -1, 3, C.addressof(bloom)) == INVALID_ARGUMENT
    assert R.same(a.FrameResult(0, 0), images[0]) and R.same(a.Result, images[0])
    _, guard = denoised_and_guard(a)
    assert (guard == 0xA5).all()
    for pt in (a, b, never):
        pt.Dispose()


def test_an_uploaded_image_round_trips_and_drives_present():
    W, H = 37, 23
    images = R.random_images(W, H)
    mine = R.random_images(W, H, seed=5)[0]; mine[3, 4, 1] = np.nan; mine[5, 6, 0] = -0.0          # any bits at all
    a, b = new_pt(W, H, aovs=False), new_pt(W, H, aovs=False)
    plant_images(a, images); write_frame(b, mine, 0)
    a.UploadDenoised(mine)
    body, guard = denoised_and_guard(a)
    assert R.same(body, mine) and (guard == 0xA5).all()
    assert a._L.idkptGetDenoiseRoute(a._ctx, -1, 0, C.byref(C.c_int32())) == INVALID_ARGUMENT      # an uploaded image ran no iteration
    a.SetResultSource(DENOISED)
    tm = T.TonemapSettings()
    a._check(c_present(a, tm, RGBA8)); b._check(c_present(b, tm, RGBA8))
    assert R.same(c_download(a, RGBA8), c_download(b, RGBA8))
    assert R.same(a.Bloom(None, 0), b.Bloom(None, 0))
    a.Dispose(); b.Dispose()


# ---- ring and lifetime
def test_ring_slots_and_what_keeps_and_releases_the_denoised_image():
    W, H = 17, 16
    s = R.settings(2, 1)
    pt = new_pt(W, H)
    pt.SetFrameRing(2)
    assert pt.BeginFrame() == 0
    im0, im1 = R.random_images(W, H, seed=1), R.random_images(W, H, seed=2)
    plant_images(pt, im0, 0); plant_images(pt, im1, 1)
    # slot 1 while slot 0 is current; -1 is the current slot
    d1 = run_case(pt, im1, s, slot=1)
    assert R.same(d1, R.denoise(*im1, **s))
    assert pt._L.idkptDownloadDenoised(pt._ctx, -1, np.zeros((H, W, 4), np.float32).ctypes.data, H * W * 16) == INVALID_OPERATION    # slot 0 has none yet
    d0 = run_case(pt, im0, s, slot=-1)
    assert R.same(d0, R.denoise(*im0, **s)) and R.same(pt.DownloadDenoised(0), d0) and R.same(pt.DownloadDenoised(1), d1)
    # kept by idkptResetAccumulation, idkptSetMaxBatch and idkptBeginFrame ("not live"); the source is a state of its own
    pt.SetResultSource(DENOISED)
    pt.ResetAccumulation(); pt.set_max_batch(4)
    assert pt.BeginFrame() == 1
    assert R.same(pt.DownloadDenoised(0), d0) and R.same(pt.DownloadDenoised(1), d1) and R.same(pt.DownloadDenoised(), d1)
    assert pt.GetResultSource() == DENOISED
    tm = T.TonemapSettings()
    assert c_present(pt, tm, RGBA8, slot=0) == 0

    def gone():
        out = np.zeros((pt.height, pt.width, 4), np.float32); p = C.c_void_p(); n = C.c_size_t()
        assert pt._L.idkptDownloadDenoised(pt._ctx, -1, out.ctypes.data, out.nbytes) == INVALID_OPERATION
        assert pt._L.idkptGetDenoisedDevicePtr(pt._ctx, -1, C.byref(p), C.byref(n)) == INVALID_OPERATION
        assert c_present(pt, tm, RGBA8) == INVALID_OPERATION and pt._L.idkptBloom(pt._ctx, -1, 0, C.addressof(T.BloomSettings())) == INVALID_OPERATION
        assert c_present(pt, tm, RGBA8, image=1) == 0                              # (images 1 and 2 do not look at the source)
        assert pt.GetResultSource() == DENOISED                                    # kept by every resize

    def again():
        plant_images(pt, im0, 0)
        assert R.same(run_case(pt, im0, s), d0) and c_present(pt, tm, RGBA8) == 0

    pt.SetFrameRing(1); gone(); again()
    pt.SetSize(W, H); gone(); again()
    # each row-layout call re-makes the images (here: back to the whole frame, so that the image can be made again)
    for call in (lambda: pt._L.idkptSetRowSharding(pt._ctx, 1, 0), lambda: pt._L.idkptSetRowBands(pt._ctx, 8, 1, 0), lambda: pt._L.idkptSetRowRange(pt._ctx, 0, H)):
        assert call() == 0
        gone(); again()
    pt.Dispose()


# ---- refusals: the status, and nothing launched
def test_refusals_leave_everything_as_it_was():
    W, H = 16, 17
    images = R.random_images(W, H)
    good = R.settings(2, 1)
    pt = new_pt(W, H)
    plant_images(pt, images)
    before = run_case(pt, images, good)
    tm = T.TonemapSettings()
    pt._check(c_present(pt, tm, RGBA8))
    shown = c_download(pt, RGBA8)

    def unchanged():
        body, guard = denoised_and_guard(pt)
        return R.same(body, before) and (guard == 0xA5).all() and R.same(c_download(pt, RGBA8), shown)

    bad = [dict(good, Iterations=0), dict(good, Iterations=9), dict(good, ColorSigma=0.0), dict(good, ColorSigma=-1.0), dict(good, ColorSigma=float("nan")), dict(good, AlbedoSigma=float("inf")),
           dict(good, AlbedoSigma=0.0), dict(good, NormalSigma=float("nan")), dict(good, NormalSigma=-0.5), dict(good, DemodulateAlbedo=2), dict(good, DemodulateAlbedo=-1)]
    for s in bad:
        assert c_denoise(pt, s) == INVALID_ARGUMENT and unchanged(), s
    L, ctx = pt._L, pt._ctx
    buf = np.zeros((H, W, 4), np.float32); p = C.c_void_p(); n = C.c_size_t(); r = C.c_int32()
    d = T.Denoise(**good)
    for slot in (-2, 1):
        assert L.idkptDenoise(ctx, slot, C.addressof(d)) == INVALID_ARGUMENT and L.idkptUploadDenoised(ctx, slot, buf.ctypes.data, buf.nbytes) == INVALID_ARGUMENT
        assert L.idkptDownloadDenoised(ctx, slot, buf.ctypes.data, buf.nbytes) == INVALID_ARGUMENT and L.idkptGetDenoisedDevicePtr(ctx, slot, C.byref(p), C.byref(n)) == INVALID_ARGUMENT
        assert L.idkptGetDenoiseRoute(ctx, slot, 0, C.byref(r)) == INVALID_ARGUMENT
    assert L.idkptDenoise(ctx, -1, None) == INVALID_ARGUMENT and L.idkptUploadDenoised(ctx, -1, None, buf.nbytes) == INVALID_ARGUMENT
    assert L.idkptDownloadDenoised(ctx, -1, None, buf.nbytes) == INVALID_ARGUMENT and L.idkptGetDenoisedDevicePtr(ctx, -1, None, None) == INVALID_ARGUMENT
    assert L.idkptGetResultSource(ctx, None) == INVALID_ARGUMENT and L.idkptGetDenoiseRoute(ctx, -1, 0, None) == INVALID_ARGUMENT
    for nbytes in (buf.nbytes - 16, buf.nbytes + 16, 0):
        assert L.idkptUploadDenoised(ctx, -1, buf.ctypes.data, nbytes) == INVALID_ARGUMENT and L.idkptDownloadDenoised(ctx, -1, buf.ctypes.data, nbytes) == INVALID_ARGUMENT
    assert L.idkptGetDenoiseRoute(ctx, -1, 2, C.byref(r)) == INVALID_ARGUMENT and L.idkptGetDenoiseRoute(ctx, -1, -1, C.byref(r)) == INVALID_ARGUMENT
    assert L.idkptSetResultSource(ctx, 2) == INVALID_ARGUMENT and L.idkptSetResultSource(ctx, -1) == INVALID_ARGUMENT and pt.GetResultSource() == NOISY
    assert unchanged()
    # OutputAOVs = 0: the guides are not accumulated
    pt.OutputAOVs = 0
    assert c_denoise(pt, good) == INVALID_OPERATION and unchanged()
    pt.Dispose()


def test_refusals_of_contexts_without_a_whole_frame():
    W, H = 16, 17
    good = T.Denoise(**R.settings(2, 1))
    buf = np.zeros((H, W, 4), np.float32)
    tm = T.TonemapSettings()
    # no size set: a raw context
    from idkengine_amd import _lib
    L = _lib.load()
    raw = C.c_void_p()
    assert L.idkptCreate(1, (C.c_int32 * 1)(0), C.byref(raw)) == 0
    assert L.idkptDenoise(raw, -1, C.addressof(good)) == INVALID_OPERATION and L.idkptUploadDenoised(raw, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
    assert L.idkptDownloadDenoised(raw, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
    assert L.idkptSetResultSource(raw, DENOISED) == 0 and L.idkptPresent(raw, -1, 0, C.addressof(tm), RGBA8, None, None) == INVALID_OPERATION
    assert L.idkptDestroy(raw) == 0
    # a two-member context and a row-band context
    group = new_pt(W, H, devices=[0, 0])
    bands = new_pt(W, H, row_modulo=2, row_remainder=1, row_band=8)
    for pt in (group, bands):
        images = R.random_images(W, H)
        pt._check(c_present(pt, tm, RGBA8))
        shown = c_download(pt, RGBA8, rows=H if pt is group else pt.rows)
        assert c_denoise(pt, good) == INVALID_OPERATION
        assert pt._L.idkptUploadDenoised(pt._ctx, -1, images[0].ctypes.data, images[0].nbytes) == INVALID_OPERATION
        assert pt._L.idkptSetResultSource(pt._ctx, DENOISED) == INVALID_OPERATION and pt.GetResultSource() == NOISY
        assert pt._L.idkptSetResultSource(pt._ctx, NOISY) == 0
        assert pt._L.idkptDownloadDenoised(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
        pt._check(c_present(pt, tm, RGBA8))
        assert R.same(c_download(pt, RGBA8, rows=H if pt is group else pt.rows), shown)
        pt.Dispose()
