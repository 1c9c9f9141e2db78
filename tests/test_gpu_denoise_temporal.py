"""Temporal moments on the device: idkptReprojectMoments and idkptDenoiseTemporal (csrc/kernels_reproject.hpp k_reproject_moments, csrc/kernels_denoise_temporal.hpp
k_temporal_state, the iterations of csrc/kernels_denoise_variance.hpp; the contract: include/idkpt.h, "temporal moments").  Everything is bit for bit: both calls against
tests/denoise_temporal_ref.py (the numpy restatement of the header's text), the filter against idkptDenoiseVariance where the two contracts coincide, the accumulated
images against a context that made none of the new calls.  The 64 guard bytes behind the temporal moments image and the denoised image are looked at after every run.

The geometry images are real captures of the small Cornell box under the cameras of tests/test_gpu_reproject.py; the synthetic cases then overwrite the temporal image,
the temporal moments, the moments, Albedo and Normal through their device pointers with a torch copy on the context's stream, as tests/test_gpu_denoise_variance.py
plants its images."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import denoise_temporal_ref as R  # noqa: E402
import denoise_variance_ref as V  # noqa: E402
import denoise_ref as D  # noqa: E402
import reproject_ref as P  # noqa: E402
from test_gpu_present import _stream, _alias, read_device, c_present, c_download  # noqa: E402
from test_gpu_denoise import denoised_and_guard  # noqa: E402
from test_gpu_reproject import CAM_A, CAMS_B, SKY, GUARD, settings_for, image_and_guard  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
NO_HISTORY = T.IDKPT_NO_HISTORY
ROUTE_NAMES = {T.IDKPT_DENOISE_ROUTE_TILED: "tiled", T.IDKPT_DENOISE_ROUTE_DIRECT: "direct"}


@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, sky_color=SKY)


def new_pt(sc, w, h, ring=2, noise=True, aovs=True, **kw):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h, **kw)
    pt.RayDepth = 3
    if aovs:
        pt.OutputAOVs = 1
    pt.UploadScene(sc)
    if ring > 1:
        pt.SetFrameRing(ring)
    if noise:
        pt.SetNoiseEstimate(True)
    return pt


def frame(pt, cam, samples):
    """BeginFrame, the camera, `samples` samples, the geometry: what a host does per frame; returns the slot"""
    slot = pt.BeginFrame()
    pt.SetCamera(cam)
    for _ in range(samples):
        pt.Compute()
    pt.CaptureGeometry()
    return slot


def write_ptr(pt, ptr_and_bytes, img):
    import torch
    img = np.ascontiguousarray(img, np.float32)
    p, n = ptr_and_bytes
    assert n == img.nbytes
    st = _stream(pt)
    with torch.cuda.stream(st):
        _alias(p, n).copy_(torch.from_numpy(img.view(np.uint8).reshape(-1)).to("cuda"))
    st.synchronize()


def plant_filter_inputs(pt, images, slot):
    """(temporal, temporal moments, Albedo, Normal) -> the slot"""
    write_ptr(pt, pt.temporal_device_ptr(slot), images[0])
    write_ptr(pt, pt.temporal_moments_device_ptr(slot), images[1])
    write_ptr(pt, pt.frame_device_ptr(slot, 1), images[2])
    write_ptr(pt, pt.frame_device_ptr(slot, 2), images[3])


def started(sc, w, h, samples=1, **kw):
    """a context whose slot 0 holds a geometry image, a temporal image and a temporal moments image (a history start): what the planted cases overwrite"""
    pt = new_pt(sc, w, h, **kw)
    assert frame(pt, S.Camera(w, h, **CAM_A), samples) == 0
    pt.Reproject(0, NO_HISTORY); pt.ReprojectMoments(0, NO_HISTORY)
    return pt


def c_temporal(pt, s, slot=-1):
    d = s if isinstance(s, T.DenoiseTemporal) else T.DenoiseTemporal(**s)
    return pt._L.idkptDenoiseTemporal(pt._ctx, slot, C.addressof(d))


def c_reproject_moments(pt, slot, history, s):
    return pt._L.idkptReprojectMoments(pt._ctx, slot, history, C.addressof(s))


def run_case(pt, s, slot=-1):
    pt._check(c_temporal(pt, s, slot))
    body, guard = denoised_and_guard(pt, slot)
    assert (guard == 0xA5).all()
    return body


def moments_and_guard(pt, slot):
    return image_and_guard(pt, pt.temporal_moments_device_ptr, pt.DownloadTemporalMoments, slot)


def guards_intact(pt, slots):
    for q in slots:
        assert (image_and_guard(pt, pt.geometry_device_ptr, pt.DownloadGeometry, q)[1] == 0xA5).all()
        assert (image_and_guard(pt, pt.temporal_device_ptr, pt.DownloadTemporal, q)[1] == 0xA5).all()
        assert (moments_and_guard(pt, q)[1] == 0xA5).all()
    return True


def differing(got, want):
    return int((R.bits(got) != R.bits(want)).any(axis=2).sum())


def history_moments(W, H, seed):
    """a planted history: moments in [0, 2), counts 1 .. 59, a few texels that are not finite and a finite z that must not reach the output"""
    rng = np.random.default_rng(seed)
    hm = (rng.random((H, W, 4)) * 2.0).astype(F); hm[..., 2] = 0.0; hm[..., 3] = rng.integers(1, 60, (H, W)).astype(F)
    hm[H // 2, W // 2, 0] = np.nan; hm[H // 3, W // 2, 3] = np.inf; hm[H // 2, W // 3, 2] = -np.inf; hm[H // 3, W // 3, 2] = 7.0
    return hm


# ---- 1. the moments reprojection on planted moments over real geometry
@pytest.mark.parametrize("size", [(64, 48), (37, 29)], ids=["64x48", "37x29"])
def test_moments_reprojection_equals_the_restatement_bit_for_bit(scene, size):
    W, H = size
    pt = new_pt(scene, W, H)
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["translation+yaw"])
    # the history start: four samples with camera A into slot 0
    assert frame(pt, cam_a, 4) == 0
    pt.ReprojectMoments(0, NO_HISTORY)
    m0 = pt.DownloadMoments(0)
    assert m0[..., 1].max() > 0 and R.same(pt.DownloadTemporalMoments(0), R.start_moments(m0, 4))
    # the camera moves: two samples into slot 1; moments and history moments planted
    assert frame(pt, cam_b, 2) == 1
    rng = np.random.default_rng(17 * W + H)
    mom = rng.random((H, W, 4)).astype(F); mom[..., 2] = 0.0; mom[..., 3] = 1.0
    hm = history_moments(W, H, W)
    write_ptr(pt, pt.moments_device_ptr(1), mom)
    write_ptr(pt, pt.temporal_moments_device_ptr(0), hm)
    g0, g1 = pt.DownloadGeometry(0), pt.DownloadGeometry(1)
    M = (cam_a.view @ cam_a.proj).astype(F)
    for s in (dict(P.DEFAULTS), dict(PositionTolerance=0.02, MaxHistory=4.0)):
        pt.ReprojectMoments(1, 0, settings_for(cam_a, **s))
        st = {}
        want = R.reproject_moments(mom, 2, g1, g0, hm, M, cam_a.position, stats=st, **s)
        got, guard = moments_and_guard(pt, 1)
        assert R.same(got, want), differing(got, want)
        assert (guard == 0xA5).all()
        assert st["history"].mean() > 0.3 and (~st["history"]).any() and st["colour"].any() and (R.bits(got[..., 2]) == 0).all()
    assert (got[..., 3] <= 6.0).all() and (got[..., 3] == 6.0).any()                 # the cap at 4, n = 2
    # the history and the slot's own inputs are read, not written
    assert R.same(pt.DownloadTemporalMoments(0), hm) and R.same(pt.DownloadMoments(1), mom) and R.same(pt.DownloadGeometry(0), g0) and R.same(pt.DownloadGeometry(1), g1)
    pt.Dispose()


# ---- 2. the count is the colour reprojection's
def test_the_count_of_the_moments_is_the_alpha_of_the_temporal_image(scene):
    W, H = 64, 48
    pt = new_pt(scene, W, H)
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["rotation"])
    assert frame(pt, cam_a, 2) == 0
    pt.ReprojectMoments(0, NO_HISTORY); pt.Reproject(0, NO_HISTORY)                  # (either order)
    rng = np.random.default_rng(23)
    cnt = rng.integers(1, 60, (H, W)).astype(F)
    hc = (rng.random((H, W, 4)) * 3.0).astype(F); hc[..., 3] = cnt
    hm = (rng.random((H, W, 4)) * 3.0).astype(F); hm[..., 2] = 0.0; hm[..., 3] = cnt
    write_ptr(pt, pt.temporal_device_ptr(0), hc); write_ptr(pt, pt.temporal_moments_device_ptr(0), hm)
    assert frame(pt, cam_b, 1) == 1
    for s in (dict(P.DEFAULTS), dict(PositionTolerance=0.02, MaxHistory=8.0)):
        sa = settings_for(cam_a, **s)
        pt.Reproject(1, 0, sa); pt.ReprojectMoments(1, 0, sa)
        t, m = pt.DownloadTemporal(1), pt.DownloadTemporalMoments(1)
        assert np.isfinite(t).all() and np.isfinite(m).all()
        assert R.same(t[..., 3], m[..., 3]) and (m[..., 3] > 1.0).mean() > 0.3 and (m[..., 3] == 1.0).any()
    assert guards_intact(pt, (0, 1))
    pt.Dispose()


# ---- 3. the filter, bit for bit
@pytest.mark.parametrize("shape", R.SHAPES, ids=[f"{w}x{h}" for w, h in R.SHAPES])
def test_denoise_temporal_equals_the_restatement_bit_for_bit(scene, shape):
    W, H = shape
    pt = started(scene, W, H)
    images = R.random_images(W, H)
    plant_filter_inputs(pt, images, 0)
    result, moments = pt.FrameResult(0, 0), pt.DownloadMoments(0)
    cases = [s for w, h, s in R.CASES if (w, h) == shape]
    assert len(cases) == 6
    for s in cases:
        got = run_case(pt, s, 0)
        want = R.denoise_temporal(*images, **s)
        assert R.same(got, want), (s, differing(got, want))
        assert [pt.denoise_route(i, 0) for i in range(s["Iterations"])] == [R.route(i) for i in range(s["Iterations"])]
    # the inputs are untouched, and so is what the call does not read
    assert R.same(pt.DownloadTemporal(0), images[0]) and R.same(pt.DownloadTemporalMoments(0), images[1]) and R.same(pt.FrameResult(0, 1), images[2]) and R.same(pt.FrameResult(0, 2), images[3])
    assert R.same(pt.FrameResult(0, 0), result) and R.same(pt.DownloadMoments(0), moments) and pt.AccumulatedSamples == 1
    assert guards_intact(pt, (0,))
    pt.Dispose()


def test_every_route_and_both_branches_are_hit_by_the_cases():
    spacings = {(ROUTE_NAMES[R.route(i)], 1 << i) for W, H, s in R.CASES if (W, H) == (64, 48) for i in range(s["Iterations"])}
    assert spacings == {("tiled", 1), ("tiled", 2), ("tiled", 4), ("direct", 8), ("direct", 16)}
    for W, H in R.SHAPES[2:]:
        br = {}
        R.first_state(*R.random_images(W, H), branch=br)
        assert br["temporal"].mean() >= 0.1 and br["spatial"].mean() >= 0.1


def test_planted_texels_stay_where_the_restatement_says(scene):
    W, H = R.PLANT_SHAPE
    clean = R.random_images(W, H)
    pt = started(scene, W, H)
    for pname, writes in R.PLANTS:
        for pos in R.PLANT_POSITIONS:
            x, y = pos
            images = R.plant(clean, writes, pos)
            plant_filter_inputs(pt, images, 0)
            for s in R.PLANT_SETTINGS:
                got = run_case(pt, s, 0)
                want = R.denoise_temporal(*images, **s)
                assert R.same(got, want), (pname, pos, s, differing(got, want))
                if not s["DemodulateAlbedo"] and writes[0][0] in (R.TEMPORAL, R.MOMENTS):
                    assert R.same(got[y, x, :3], images[0][y, x, :3]), (pname, pos)      # the planted pixel keeps its temporal rgb
    pt.Dispose()


# ---- 4. where the two contracts coincide, the two filters do
def test_with_a_uniform_integer_count_the_filter_is_denoise_variance(scene):
    W, H, N = 37, 29, 4
    pt = started(scene, W, H, samples=N)
    assert pt.AccumulatedSamples == N
    result, albedo, normal, moments = V.random_images(W, H, N=N)
    for i, im in enumerate((result, albedo, normal)):
        write_ptr(pt, pt.frame_device_ptr(0, i), im)
    write_ptr(pt, pt.moments_device_ptr(0), moments)
    temporal = result.copy(); temporal[..., 3] = 77.0                                # (the alpha of the temporal image is not read)
    tm = moments.copy(); tm[..., 2] = 0.0; tm[..., 3] = F(N)
    write_ptr(pt, pt.temporal_device_ptr(0), temporal); write_ptr(pt, pt.temporal_moments_device_ptr(0), tm)
    plain = T.Denoise()
    for demod in (0, 1):
        sv = V.settings(5, demod)
        d = T.DenoiseVariance(**sv)
        pt._check(pt._L.idkptDenoiseVariance(pt._ctx, 0, C.addressof(d)))
        pinned = denoised_and_guard(pt, 0)[0].copy()
        assert R.same(pinned, V.denoise_variance(result, albedo, normal, moments, N, **sv))
        pt._check(pt._L.idkptDenoise(pt._ctx, 0, C.addressof(plain)))                # (another picture in between)
        assert not R.same(denoised_and_guard(pt, 0)[0], pinned)
        got = run_case(pt, dict(sv, SpatialBelow=float(N)), 0)
        assert R.same(got, pinned), (demod, differing(got, pinned))
        # the new filter ignores idkptSetDenoiseInput
        pt.SetDenoiseInput(T.IDKPT_DENOISE_INPUT_TEMPORAL)
        assert R.same(run_case(pt, dict(sv, SpatialBelow=float(N)), 0), pinned)
        assert pt._L.idkptDenoiseVariance(pt._ctx, 0, C.addressof(d)) == INVALID_OPERATION      # (the pinned refusal stays)
        pt.SetDenoiseInput(T.IDKPT_DENOISE_INPUT_ACCUMULATED)
    pt.Dispose()


def test_the_fillers_in_any_order_on_one_slot(scene):
    """Every call that fills the denoised image of a slot, one behind the other on ONE slot, so that each meets the ping images a different filler left present or absent
    (idkptDenoise and idkptDenoiseVariance make ping[0] from 2 iterations and ping[1] from 3, idkptDenoiseTemporal ping[1] always and ping[0] from 2, idkptUploadDenoised
    neither): each image is its own restatement's bit for bit, idkptGetDenoiseRoute answers for exactly that call's iterations, and no guard is touched."""
    W, H, N = 37, 23, 2
    pt = started(scene, W, H, samples=N)
    assert pt.AccumulatedSamples == N
    result, _, _, moments = V.random_images(W, H, N=N)
    temporal, tm, albedo, normal = R.random_images(W, H)
    write_ptr(pt, pt.frame_device_ptr(0, 0), result); write_ptr(pt, pt.moments_device_ptr(0), moments)
    plant_filter_inputs(pt, (temporal, tm, albedo, normal), 0)
    uploaded = np.random.default_rng(5).random((H, W, 4)).astype(F)

    def plain(it, demod):
        s = D.settings(it, demod); d = T.Denoise(**s)
        pt._check(pt._L.idkptDenoise(pt._ctx, 0, C.addressof(d)))
        return D.denoise(result, albedo, normal, **s), it

    def variance(it, demod):
        s = V.settings(it, demod); d = T.DenoiseVariance(**s)
        pt._check(pt._L.idkptDenoiseVariance(pt._ctx, 0, C.addressof(d)))
        return V.denoise_variance(result, albedo, normal, moments, N, **s), it

    def temporal_filter(it, demod):
        s = R.settings(it, demod)
        pt._check(c_temporal(pt, s, 0))
        return R.denoise_temporal(temporal, tm, albedo, normal, **s), it

    def upload():
        pt.UploadDenoised(uploaded, 0)
        return uploaded, 0

    steps = [("Denoise 1", lambda: plain(1, 1)), ("DenoiseTemporal 1", lambda: temporal_filter(1, 0)), ("DenoiseVariance 2", lambda: variance(2, 1)), ("Denoise 3", lambda: plain(3, 0)),
             ("UploadDenoised", upload), ("DenoiseTemporal 2", lambda: temporal_filter(2, 1)), ("DenoiseVariance 1", lambda: variance(1, 0))]
    r = C.c_int32()
    for name, step in steps:
        want, it = step()
        got, guard = denoised_and_guard(pt, 0)
        assert R.same(got, want), (name, differing(got, want))
        assert (guard == 0xA5).all(), name
        assert [pt.denoise_route(i, 0) for i in range(it)] == [R.route(i) for i in range(it)], name
        assert pt._L.idkptGetDenoiseRoute(pt._ctx, 0, it, C.byref(r)) == INVALID_ARGUMENT, name      # exactly that call's iterations: none past them
        assert guards_intact(pt, (0,)), name
    # the inputs are read, not written
    assert R.same(pt.FrameResult(0, 0), result) and R.same(pt.DownloadMoments(0), moments) and R.same(pt.DownloadTemporal(0), temporal) and R.same(pt.DownloadTemporalMoments(0), tm)
    assert R.same(pt.FrameResult(0, 1), albedo) and R.same(pt.FrameResult(0, 2), normal)
    pt.Dispose()


# ---- 5. end to end: eight one-sample frames along a camera path
def path_camera(W, H, k, frames=8):
    a, b = CAM_A, CAMS_B["rotation"]                     # about 1.4 pixels per frame: new columns enter every frame, so counts below SpatialBelow exist in every frame
    f = k / float(frames - 1)
    mix = lambda u, v: tuple(float(p + (q - p) * f) for p, q in zip(u, v))
    return S.Camera(W, H, position=mix(a["position"], b["position"]), view_dir=mix(a["view_dir"], b["view_dir"]), fovy_deg=90.0)


def test_eight_frames_end_to_end_and_nothing_else_notices(scene):
    W, H = 64, 48
    new, old = new_pt(scene, W, H), new_pt(scene, W, H)
    prev, prev_cam, hm, hg = NO_HISTORY, None, None, None
    took = []
    for k in range(8):
        cam = path_camera(W, H, k)
        s = T.Reproject() if prev_cam is None else settings_for(prev_cam)
        for pt in (new, old):
            slot = frame(pt, cam, 1)
            pt.Reproject(slot, prev, s)
        new.ReprojectMoments(slot, prev, s)
        den = new.DenoiseTemporal(slot=slot)
        mom, g, tm = new.DownloadMoments(slot), new.DownloadGeometry(slot), new.DownloadTemporalMoments(slot)
        if prev == NO_HISTORY:
            want = R.start_moments(mom, 1)
        else:
            want = R.reproject_moments(mom, 1, g, hg, hm, (prev_cam.view @ prev_cam.proj).astype(F), prev_cam.position, **P.DEFAULTS)
        assert R.same(tm, want), (k, differing(tm, want))
        temporal = new.DownloadTemporal(slot)
        assert R.same(tm[..., 3], temporal[..., 3]), k
        inputs = (temporal, tm, new.FrameResult(slot, 1), new.FrameResult(slot, 2))
        want = R.denoise_temporal(*inputs, **R.DEFAULTS)
        assert R.same(den, want), (k, differing(den, want))
        took.append(float((tm[..., 3] > 1.0).mean()))
        # everything the old calls make is what it is without the new ones
        for image in range(3):
            assert R.same(new.FrameResult(slot, image), old.FrameResult(slot, image)), (k, image)
        assert R.same(mom, old.DownloadMoments(slot)) and R.same(g, old.DownloadGeometry(slot)) and R.same(temporal, old.DownloadTemporal(slot))
        assert new.AccumulatedSamples == old.AccumulatedSamples == 1
        prev, prev_cam, hm, hg = slot, cam, tm, g
    assert min(took[1:]) > 0.5 and tm[..., 3].max() > 4.0                            # the history was found, and grew past SpatialBelow
    br = {}
    R.first_state(*inputs, branch=br)
    assert br["temporal"].any() and br["spatial"].any()
    assert not R.same(den[..., :3], temporal[..., :3])
    # the pinned filters answer as before: a two-sample frame in both contexts
    for pt in (new, old):
        slot = frame(pt, cam, 2)
    assert R.same(new.Denoise(slot=slot), old.Denoise(slot=slot))
    assert R.same(new.DenoiseVariance(slot=slot), old.DenoiseVariance(slot=slot))
    assert guards_intact(new, (0, 1))
    assert (denoised_and_guard(new, 0)[1] == 0xA5).all() and (denoised_and_guard(new, 1)[1] == 0xA5).all()
    new.Dispose(); old.Dispose()


# ---- 6. guards, life cycle, refusals, the result source
def test_present_shows_the_new_image_while_the_source_says_so(scene):
    W, H = 37, 29
    images = list(R.random_images(W, H)); images[0] = images[0].copy(); images[0][..., :3] *= 4.0
    s = R.settings(3, 1)
    tm_settings = T.TonemapSettings()
    a, b = started(scene, W, H), new_pt(scene, W, H, noise=False)
    b.SetCamera(S.Camera(W, H, **CAM_A)); b.BeginFrame(); b.Compute()
    plant_filter_inputs(a, images, 0)
    den = run_case(a, s, 0)
    assert R.same(den, R.denoise_temporal(*images, **s))
    b.UploadDenoised(den)                                                        # the same bytes through idkptUploadDenoised
    for fmt in (T.IDKPT_DISPLAY_RGBA8, T.IDKPT_DISPLAY_RGBA32F):
        a._check(c_present(a, tm_settings, fmt)); noisy = c_download(a, fmt)
        a.SetResultSource(T.IDKPT_RESULT_DENOISED); b.SetResultSource(T.IDKPT_RESULT_DENOISED)
        a._check(c_present(a, tm_settings, fmt)); b._check(c_present(b, tm_settings, fmt))
        assert R.same(c_download(a, fmt), c_download(b, fmt)) and not R.same(c_download(a, fmt), noisy)
        a.SetResultSource(T.IDKPT_RESULT_NOISY); b.SetResultSource(T.IDKPT_RESULT_NOISY)
    a.Dispose(); b.Dispose()


def test_the_moments_image_survives_what_the_temporal_image_survives_and_the_noise_switch(scene):
    W, H = 64, 48
    pt = new_pt(scene, W, H)
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["translation+yaw"])
    frame(pt, cam_a, 2); pt.Reproject(0, NO_HISTORY); pt.ReprojectMoments(0, NO_HISTORY)
    frame(pt, cam_b, 1); pt.Reproject(1, 0, settings_for(cam_a)); pt.ReprojectMoments(1, 0, settings_for(cam_a))
    kept = [pt.DownloadTemporalMoments(q) for q in (0, 1)]
    assert (kept[1][..., 3] > 1.0).mean() > 0.5
    pt.ResetAccumulation(); pt.set_max_batch(4); pt.SetPresentationSize(32, 32)
    assert pt.BeginFrame() == 0
    pt.SetNoiseEstimate(False)
    for q in (0, 1):
        assert R.same(pt.DownloadTemporalMoments(q), kept[q])
    # with the switch off the filter still runs on what the slot holds; the reprojection of moments is refused
    pt.DenoiseTemporal(slot=1)
    pt.SetCamera(cam_b); pt.Compute(); pt.CaptureGeometry()
    assert c_reproject_moments(pt, 0, 1, settings_for(cam_b)) == INVALID_OPERATION
    pt.SetNoiseEstimate(True)
    for q in (0, 1):
        assert R.same(pt.DownloadTemporalMoments(q), kept[q])
    # surviving is the point: the next frame reprojects onto the kept history
    pt.Compute(); pt.CaptureGeometry()
    pt.ReprojectMoments(0, 1, settings_for(cam_b))
    assert (pt.DownloadTemporalMoments(0)[..., 3] > 1.0).mean() > 0.5
    pt.Reproject(0, 1, settings_for(cam_b))
    assert guards_intact(pt, (0, 1))

    def gone():
        buf = np.zeros((pt.height, pt.width, 4), np.float32); p = C.c_void_p(); n = C.c_size_t()
        d = T.DenoiseTemporal()
        for q in (0, 1):
            assert pt._L.idkptDownloadTemporalMoments(pt._ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
            assert pt._L.idkptGetTemporalMomentsDevicePtr(pt._ctx, q, C.byref(p), C.byref(n)) == INVALID_OPERATION
            assert pt._L.idkptDenoiseTemporal(pt._ctx, q, C.addressof(d)) == INVALID_OPERATION

    pt.SetSize(W, H); gone()
    pt.SetCamera(cam_a); pt.Compute(); pt.CaptureGeometry(); pt.Reproject(None, NO_HISTORY); pt.ReprojectMoments(None, NO_HISTORY)
    assert (moments_and_guard(pt, None)[1] == 0xA5).all()
    pt.SetFrameRing(3); gone()
    pt.Dispose()


def test_refusals_leave_the_previous_images_as_they_were(scene):
    W, H = 37, 29
    pt = new_pt(scene, W, H)
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["translation+yaw"])
    frame(pt, cam_a, 2); pt.Reproject(0, NO_HISTORY); pt.ReprojectMoments(0, NO_HISTORY)
    frame(pt, cam_b, 1); pt.Reproject(1, 0, settings_for(cam_a)); pt.ReprojectMoments(1, 0, settings_for(cam_a))
    good = R.settings(2, 1)
    den = run_case(pt, good, 1)
    before = [pt.DownloadTemporalMoments(q) for q in (0, 1)]

    def unchanged():
        body, guard = denoised_and_guard(pt, 1)
        return R.same(body, den) and (guard == 0xA5).all() and all(R.same(pt.DownloadTemporalMoments(q), before[q]) for q in (0, 1)) and guards_intact(pt, (0, 1))

    nan, inf = float("nan"), float("inf")
    # idkptDenoiseTemporal: arguments
    bad = [dict(good, Iterations=0), dict(good, Iterations=9), dict(good, LumaSigma=0.0), dict(good, LumaSigma=nan), dict(good, LumaSigma=inf), dict(good, VarianceEpsilon=0.0),
           dict(good, VarianceEpsilon=-1e-3), dict(good, VarianceEpsilon=nan), dict(good, AlbedoSigma=inf), dict(good, AlbedoSigma=0.0), dict(good, NormalSigma=nan), dict(good, NormalSigma=-0.5),
           dict(good, DemodulateAlbedo=2), dict(good, DemodulateAlbedo=-1), dict(good, SpatialBelow=1.5), dict(good, SpatialBelow=nan), dict(good, SpatialBelow=inf), dict(good, SpatialBelow=-4.0)]
    for s in bad:
        assert c_temporal(pt, s, 1) == INVALID_ARGUMENT, s
    d = T.DenoiseTemporal(**good)
    for slot in (-2, 2):
        assert pt._L.idkptDenoiseTemporal(pt._ctx, slot, C.addressof(d)) == INVALID_ARGUMENT
    assert pt._L.idkptDenoiseTemporal(pt._ctx, 1, None) == INVALID_ARGUMENT and pt._L.idkptDenoiseTemporal(None, 1, C.addressof(d)) == INVALID_ARGUMENT
    assert c_temporal(pt, dict(good, SpatialBelow=2.0), 1) == 0 and c_temporal(pt, good, 1) == 0 and unchanged()      # (2 is in range; the same call is accepted again)
    # idkptReprojectMoments: idkptReproject's argument checks
    for b in (dict(PositionTolerance=0.0), dict(PositionTolerance=nan), dict(PositionTolerance=inf), dict(MaxHistory=0.5), dict(MaxHistory=nan), dict(MaxHistory=inf)):
        assert c_reproject_moments(pt, 1, 0, settings_for(cam_a, **dict(P.DEFAULTS, **b))) == INVALID_ARGUMENT, b
    sa = settings_for(cam_a)
    assert c_reproject_moments(pt, 1, 1, sa) == INVALID_ARGUMENT and c_reproject_moments(pt, -1, 1, sa) == INVALID_ARGUMENT      # slot == historySlot (-1 is slot 1 here)
    for slot, hist in ((2, 0), (-2, 0), (1, 2), (1, -1), (1, -3)):
        assert c_reproject_moments(pt, slot, hist, sa) == INVALID_ARGUMENT, (slot, hist)
    assert pt._L.idkptReprojectMoments(pt._ctx, 1, 0, None) == INVALID_ARGUMENT
    buf = np.zeros((H, W, 4), np.float32); p = C.c_void_p(); n = C.c_size_t()
    L, ctx = pt._L, pt._ctx
    for q in (-2, 2):
        assert L.idkptDownloadTemporalMoments(ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_ARGUMENT and L.idkptGetTemporalMomentsDevicePtr(ctx, q, C.byref(p), C.byref(n)) == INVALID_ARGUMENT
    for nbytes in (buf.nbytes - 16, buf.nbytes + 16, 0):
        assert L.idkptDownloadTemporalMoments(ctx, 0, buf.ctypes.data, nbytes) == INVALID_ARGUMENT
    assert L.idkptDownloadTemporalMoments(ctx, 0, None, buf.nbytes) == INVALID_ARGUMENT and L.idkptGetTemporalMomentsDevicePtr(ctx, 0, None, None) == INVALID_ARGUMENT
    assert unchanged()
    # OutputAOVs = 0: the guides are not accumulated
    pt.OutputAOVs = 0
    assert c_temporal(pt, good, 1) == INVALID_OPERATION and unchanged()
    pt.OutputAOVs = 1
    # the noise switch off: no moments to reproject (the filter needs no switch)
    pt.SetNoiseEstimate(False)
    pt.Compute()
    assert c_reproject_moments(pt, 1, 0, sa) == INVALID_OPERATION and c_reproject_moments(pt, 1, NO_HISTORY, sa) == INVALID_OPERATION and unchanged()
    assert c_temporal(pt, good, 1) == 0 and unchanged()
    pt.SetNoiseEstimate(True)
    # n == 0: a frame that has begun and rendered nothing
    assert pt.BeginFrame() == 0
    assert c_reproject_moments(pt, 0, 1, sa) == INVALID_OPERATION and unchanged()
    pt.Dispose()
    # no geometry in either slot; no temporal moments image in the history slot; the filter without one image or the other
    pt = new_pt(scene, W, H)
    d = T.DenoiseTemporal()
    pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute()
    assert c_reproject_moments(pt, 0, NO_HISTORY, sa) == INVALID_OPERATION                    # slot 0 without geometry
    pt.CaptureGeometry()
    assert pt._L.idkptDenoiseTemporal(pt._ctx, 0, C.addressof(d)) == INVALID_OPERATION         # neither image
    pt.Reproject(0, NO_HISTORY)
    assert pt._L.idkptDenoiseTemporal(pt._ctx, 0, C.addressof(d)) == INVALID_OPERATION         # a temporal image, no temporal moments
    pt.BeginFrame(); pt.Compute()
    assert c_reproject_moments(pt, 1, 0, sa) == INVALID_OPERATION                              # slot 1 without geometry
    pt.CaptureGeometry()
    assert c_reproject_moments(pt, 1, 0, sa) == INVALID_OPERATION                              # the history slot has geometry and no temporal moments
    pt.ReprojectMoments(0, NO_HISTORY)
    assert c_reproject_moments(pt, 1, 0, sa) == 0
    assert pt._L.idkptDenoiseTemporal(pt._ctx, 1, C.addressof(d)) == INVALID_OPERATION         # temporal moments, no temporal image
    assert pt._L.idkptDownloadDenoised(pt._ctx, 1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION      # (no refused call made a denoised image)
    pt.Reproject(1, 0, sa)
    assert pt._L.idkptDenoiseTemporal(pt._ctx, 1, C.addressof(d)) == 0
    pt.Dispose()
    # no size set; a two-member context and a row-band context
    from idkengine_amd import _lib
    from idkengine_amd.pathtracer import PathTracer
    L = _lib.load()
    raw = C.c_void_p()
    assert L.idkptCreate(1, (C.c_int32 * 1)(0), C.byref(raw)) == 0
    assert L.idkptReprojectMoments(raw, 0, NO_HISTORY, C.addressof(sa)) == INVALID_OPERATION and L.idkptDenoiseTemporal(raw, -1, C.addressof(d)) == INVALID_OPERATION
    assert L.idkptDownloadTemporalMoments(raw, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
    assert L.idkptDestroy(raw) == 0
    for kw in (dict(devices=[0, 0]), dict(row_modulo=2, row_remainder=1, row_band=8)):
        pt = PathTracer(W, H, **kw)
        pt.UploadScene(scene); pt.SetCamera(cam_a); pt.Compute()
        assert c_reproject_moments(pt, 0, NO_HISTORY, sa) == INVALID_OPERATION and pt._L.idkptDenoiseTemporal(pt._ctx, -1, C.addressof(d)) == INVALID_OPERATION
        assert pt._L.idkptDownloadTemporalMoments(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
        pt.Dispose()
