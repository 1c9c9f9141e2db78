"""Temporal reprojection on the device: idkptCaptureGeometry, idkptReproject, idkptUseTemporalAsDenoised and idkptSetDenoiseInput (csrc/kernels_reproject.hpp,
csrc/host_reproject.hpp; the contract: include/idkpt.h).  Everything is bit for bit: the geometry image against the restated pack (tests/reproject_ref.py) of idkptTraceRays
hits for centre rays made with the oracle's GetWorldSpaceDirection (tests/c_driver/reproject_host.cpp, mode "rays"); the temporal image against the restatement fed the
downloaded Result, geometries and history; the consumers against the calls they stand in for.  The 64 guard bytes behind both images are looked at after every sequence.

The scene is the Cornell box seen from inside, looking out of its open side at the sky; the cameras were chosen on the CPU from oracle hits so that the restatement alone
shows what each case must show (the assertions on `stats` below): history on at least half of the pixels in the first two cases, and every rejection rule — off-screen,
id mismatch, position, clip.w — deciding some pixel somewhere in the three."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import reproject_ref as R  # noqa: E402
import denoise_ref as DR  # noqa: E402
from test_gpu_present import read_device, c_present, c_download  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
GUARD = 64
SIZES = [(64, 64), (70, 37)]                       # whole 16 x 16 tiles; no multiple of 16 or of 8 in either axis
SKY = (0.4, 0.6, 0.9)
CAM_A = dict(position=(0.1, 0.0, -0.6), view_dir=(0.0, 0.0, 1.0), fovy_deg=90.0)
CAMS_B = {"translation+yaw": dict(position=(0.15, 0.02, -0.55), view_dir=(0.05, 0.0, 1.0), fovy_deg=90.0),
          "rotation": dict(position=(0.1, 0.0, -0.6), view_dir=(0.25, 0.1, 1.0), fovy_deg=90.0),
          "mostly-new-view": dict(position=(0.0, 0.0, -0.8), view_dir=(0.8, 0.0, 1.0), fovy_deg=90.0)}   # over a third of the frame was not in A's view, part of it behind A


@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, sky_color=SKY)


@pytest.fixture(scope="module")
def ray_program(tmp_path_factory):
    """the oracle's GetWorldSpaceDirection as a program (no sanitizer here: tests/test_reproject_ref.py runs it under ASan/UBSan)"""
    return R.build_host_program(str(tmp_path_factory.mktemp("reproject_rays") / "reproject_host"), sanitize=False)


def new_pt(sc, w, h, ring=2):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h)
    pt.OutputAOVs = 1; pt.RayDepth = 3
    pt.UploadScene(sc)
    if ring > 1:
        pt.SetFrameRing(ring)
    return pt


def settings_for(cam, **kw):
    return T.Reproject.from_camera(cam, **kw)


def c_reproject(pt, slot, history, s):
    return pt._L.idkptReproject(pt._ctx, slot, history, C.addressof(s))


def image_and_guard(pt, ptr_fn, download, slot):
    p, n = ptr_fn(slot)
    assert n == pt.height * pt.width * 16
    raw = read_device(pt, p, n + GUARD)
    body = raw[:n].view(np.float32).reshape(pt.height, pt.width, 4)
    assert R.same(body, download(slot))                   # the device pointer equals the download
    return body, raw[n:]


def guards_intact(pt, slots):
    for q in slots:
        assert (image_and_guard(pt, pt.geometry_device_ptr, pt.DownloadGeometry, q)[1] == 0xA5).all()
        assert (image_and_guard(pt, pt.temporal_device_ptr, pt.DownloadTemporal, q)[1] == 0xA5).all()
    return True


def frame(pt, cam, samples):
    """BeginFrame, the camera, `samples` samples, the geometry: what a host does per frame; returns the slot"""
    slot = pt.BeginFrame()
    pt.SetCamera(cam)
    for _ in range(samples):
        pt.Compute()
    pt.CaptureGeometry()
    return slot


# ---- the geometry image
@pytest.mark.parametrize("size", SIZES, ids=["64x64", "70x37"])
def test_geometry_equals_the_restated_pack_of_traced_centre_rays(scene, ray_program, tmp_path, size):
    W, H = size
    pt = new_pt(scene, W, H)
    for name, kw in [("A", CAM_A)] + list(CAMS_B.items()):
        cam = S.Camera(W, H, **kw)
        slot = frame(pt, cam, 1)
        o, d = R.oracle_centre_rays(ray_program, str(tmp_path), cam.inv_projection, cam.inv_view, W, H)
        rays = np.zeros(W * H, T.RayQuery); rays["Origin"] = o; rays["Direction"] = d.reshape(-1, 3); rays["MaxDist"] = R.FLT_MAX
        hits = pt.TraceRays(rays)
        want = R.pack(o, d, hits["T"].reshape(H, W), hits["MeshTransformId"].reshape(H, W), hits["Hit"].reshape(H, W))
        got, guard = image_and_guard(pt, pt.geometry_device_ptr, pt.DownloadGeometry, slot)
        assert R.same(got, want), (name, int((R.bits(got) != R.bits(want)).any(axis=2).sum()))
        miss = R.bits(got[..., 3]) == 0xFFFFFFFF
        assert miss.any() and (~miss).any() and (hits["Hit"].reshape(H, W) == 0)[miss].all(), name     # hit and miss pixels are both present
        assert (guard == 0xA5).all()
    pt.Dispose()


# ---- the reprojection sequence
@pytest.fixture(scope="module")
def rule_counts():
    return {}


@pytest.mark.parametrize("size", SIZES, ids=["64x64", "70x37"])
@pytest.mark.parametrize("case", list(CAMS_B), ids=list(CAMS_B))
def test_reprojection_equals_the_restatement_bit_for_bit(scene, rule_counts, case, size):
    W, H = size
    pt = new_pt(scene, W, H)
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B[case])
    # 1. four samples with camera A into slot 0, capture, start a history
    assert frame(pt, cam_a, 4) == 0
    pt.Reproject(0, T.IDKPT_NO_HISTORY)
    result0, g0, t0 = pt.FrameResult(0), pt.DownloadGeometry(0), pt.DownloadTemporal(0)
    assert R.same(t0, R.start(result0, 4))
    # 2. the camera moves: one sample into slot 1, capture, reproject onto slot 0
    assert frame(pt, cam_b, 1) == 1
    sa = settings_for(cam_a)
    pt.Reproject(1, 0, sa)
    result1, g1 = pt.FrameResult(1), pt.DownloadGeometry(1)
    st = {}
    want = R.reproject(result1, 1, g1, g0, t0, (cam_a.view @ cam_a.proj).astype(np.float32), cam_a.position, stats=st, **R.DEFAULTS)
    got = pt.DownloadTemporal(1)
    assert R.same(got, want), int((R.bits(got) != R.bits(want)).any(axis=2).sum())
    assert R.same(pt.DownloadTemporal(0), t0) and R.same(pt.DownloadGeometry(0), g0)          # the history is read, not written
    # nothing passes vacuously
    if case != "mostly-new-view":
        assert st["history"].mean() >= 0.5, st["history"].mean()
    else:
        assert (st["offscreen"] | st["clip_w"]).mean() >= 1.0 / 3.0
    assert st["history"].any() and (want[..., 3][st["history"]] > 1.0).all() and (want[..., 3][~st["history"]] == 1.0).all()
    for k in ("offscreen", "id", "position", "clip_w"):
        rule_counts[k] = rule_counts.get(k, 0) + int(st[k].sum())
    # 3. a third frame, back in slot 0, with the cap at 4: alpha <= 4 + n everywhere
    assert frame(pt, cam_b, 2) == 0
    sb = settings_for(cam_b, MaxHistory=4.0)
    pt.Reproject(0, 1, sb)
    third = pt.DownloadTemporal(0)
    want3 = R.reproject(pt.FrameResult(0), 2, pt.DownloadGeometry(0), g1, got, (cam_b.view @ cam_b.proj).astype(np.float32), cam_b.position, PositionTolerance=0.02, MaxHistory=4.0)
    assert R.same(third, want3) and (third[..., 3] <= 6.0).all() and (third[..., 3] == 6.0).any()
    assert guards_intact(pt, (0, 1))
    pt.Dispose()


def test_every_rejection_rule_decided_some_pixel(rule_counts):
    """(runs behind the parametrised sequence above, whose restatement runs it sums up)"""
    assert set(rule_counts) == {"offscreen", "id", "position", "clip_w"} and all(v > 0 for v in rule_counts.values()), rule_counts


# ---- the consumers
def sequence(pt, W, H):
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["translation+yaw"])
    frame(pt, cam_a, 2); pt.Reproject(0, T.IDKPT_NO_HISTORY)
    frame(pt, cam_b, 1); pt.Reproject(1, 0, settings_for(cam_a))
    return cam_a, cam_b


def test_the_temporal_image_reaches_present_and_denoise(scene):
    W, H = 70, 37
    a, b = new_pt(scene, W, H), new_pt(scene, W, H, ring=1)
    sequence(a, W, H)
    temporal = a.DownloadTemporal(1)
    # UseTemporalAsDenoised + Present under RESULT_DENOISED == Present of an UploadDenoised of the same pixels
    a.UseTemporalAsDenoised(1)
    shown = temporal.copy(); shown[..., 3] = 1.0
    assert R.same(a.DownloadDenoised(1), shown)
    b.UploadDenoised(shown)
    tm = T.TonemapSettings()
    for pt in (a, b):
        pt.SetResultSource(T.IDKPT_RESULT_DENOISED)
    for fmt in (T.IDKPT_DISPLAY_RGBA8, T.IDKPT_DISPLAY_RGBA32F):
        a._check(c_present(a, tm, fmt, slot=1)); b._check(c_present(b, tm, fmt))
        assert R.same(c_download(a, fmt, slot=1), c_download(b, fmt))
    assert R.same(a.Bloom(None, 0, 1), b.Bloom(None, 0))
    # idkptDenoise under INPUT_TEMPORAL == the restated filter on the temporal rgb; guides and everything else as before
    images = [a.FrameResult(1, i) for i in range(3)]
    plain = a.Denoise(slot=1)
    assert R.same(plain, DR.denoise(*images, **DR.DEFAULTS))
    assert a.GetDenoiseInput() == T.IDKPT_DENOISE_INPUT_ACCUMULATED
    a.SetDenoiseInput(T.IDKPT_DENOISE_INPUT_TEMPORAL)
    assert a.GetDenoiseInput() == T.IDKPT_DENOISE_INPUT_TEMPORAL
    got = a.Denoise(slot=1)
    assert R.same(got, DR.denoise(temporal, images[1], images[2], **DR.DEFAULTS)) and not R.same(got, plain)
    # idkptDenoiseVariance under INPUT_TEMPORAL is refused (and the denoised image stays)
    a.SetNoiseEstimate(True)                             # (restarts the accumulation; the temporal image survives)
    a.SetCamera(S.Camera(W, H, **CAMS_B["translation+yaw"]))
    for _ in range(2):
        a.Compute()
    dv = T.DenoiseVariance()
    assert a._L.idkptDenoiseVariance(a._ctx, 1, C.addressof(dv)) == INVALID_OPERATION and R.same(a.DownloadDenoised(1), got)
    a.SetDenoiseInput(T.IDKPT_DENOISE_INPUT_ACCUMULATED)
    assert a._L.idkptDenoiseVariance(a._ctx, 1, C.addressof(dv)) == 0
    # a slot without a temporal image refuses the temporal input
    a.SetDenoiseInput(T.IDKPT_DENOISE_INPUT_TEMPORAL)
    c = new_pt(scene, W, H)
    c.SetDenoiseInput(T.IDKPT_DENOISE_INPUT_TEMPORAL)
    d = T.Denoise()
    assert c._L.idkptDenoise(c._ctx, -1, C.addressof(d)) == INVALID_OPERATION and c._L.idkptUseTemporalAsDenoised(c._ctx, -1) == INVALID_OPERATION
    assert c._L.idkptSetDenoiseInput(c._ctx, 2) == INVALID_ARGUMENT and c._L.idkptSetDenoiseInput(c._ctx, -1) == INVALID_ARGUMENT and c.GetDenoiseInput() == T.IDKPT_DENOISE_INPUT_TEMPORAL
    assert guards_intact(a, (0, 1))
    for pt in (a, b, c):
        pt.Dispose()


# ---- invariance: the accumulated images and the count never notice
def test_the_accumulation_is_bit_identical_with_and_without_the_new_calls(scene):
    W, H = 70, 37
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["rotation"])
    with_calls, without = new_pt(scene, W, H), new_pt(scene, W, H)
    for pt in (with_calls, without):
        pt.set_max_batch(2)                              # (samples stay queued between calls: the new calls launch them first)
    for pt, calls in ((with_calls, True), (without, False)):
        pt.BeginFrame(); pt.SetCamera(cam_a)
        pt.Compute(); pt.Compute(); pt.Compute()
        if calls:
            pt.CaptureGeometry(); pt.Reproject(0, T.IDKPT_NO_HISTORY)
        pt.Compute()
        pt.BeginFrame(); pt.SetCamera(cam_b)
        pt.Compute()
        if calls:
            pt.CaptureGeometry(); pt.Reproject(1, 0, settings_for(cam_a)); pt.UseTemporalAsDenoised(1)
        pt.Compute(); pt.Compute()
        if calls:
            pt.CaptureGeometry(); pt.Reproject(1, 0, settings_for(cam_a))
    for slot in (0, 1):
        for image in range(3):
            assert R.same(with_calls.FrameResult(slot, image), without.FrameResult(slot, image)), (slot, image)
    assert with_calls.AccumulatedSamples == without.AccumulatedSamples == 3
    assert np.abs(with_calls.FrameResult(1, 1)[..., :3]).max() > 0
    assert guards_intact(with_calls, (0, 1))
    for pt in (with_calls, without):
        pt.Dispose()


# ---- refusals: the status, and the previous image stays
def test_refusals_leave_the_previous_temporal_image(scene):
    W, H = 64, 64
    pt = new_pt(scene, W, H)
    cam_a, _ = sequence(pt, W, H)
    before = [pt.DownloadTemporal(q) for q in (0, 1)]
    good = dict(PositionTolerance=0.02, MaxHistory=32.0)

    def unchanged():
        return all(R.same(pt.DownloadTemporal(q), before[q]) for q in (0, 1)) and guards_intact(pt, (0, 1))

    for bad in (dict(good, PositionTolerance=0.0), dict(good, PositionTolerance=-1.0), dict(good, PositionTolerance=float("nan")), dict(good, PositionTolerance=float("inf")),
                dict(good, MaxHistory=0.5), dict(good, MaxHistory=float("nan")), dict(good, MaxHistory=float("inf")), dict(good, MaxHistory=-3.0)):
        assert c_reproject(pt, 1, 0, settings_for(cam_a, **bad)) == INVALID_ARGUMENT, bad
    s = settings_for(cam_a)
    assert c_reproject(pt, 1, 1, s) == INVALID_ARGUMENT and c_reproject(pt, -1, 1, s) == INVALID_ARGUMENT          # slot == historySlot (-1 is slot 1 here)
    for slot, hist in ((2, 0), (-2, 0), (1, 2), (1, -1), (1, -3)):
        assert c_reproject(pt, slot, hist, s) == INVALID_ARGUMENT, (slot, hist)
    assert pt._L.idkptReproject(pt._ctx, 1, 0, None) == INVALID_ARGUMENT
    buf = np.zeros((H, W, 4), np.float32); p = C.c_void_p(); n = C.c_size_t()
    L, ctx = pt._L, pt._ctx
    for q in (-2, 2):
        assert L.idkptCaptureGeometry(ctx, q) == INVALID_ARGUMENT and L.idkptDownloadGeometry(ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_ARGUMENT
        assert L.idkptDownloadTemporal(ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_ARGUMENT and L.idkptUseTemporalAsDenoised(ctx, q) == INVALID_ARGUMENT
        assert L.idkptGetGeometryDevicePtr(ctx, q, C.byref(p), C.byref(n)) == INVALID_ARGUMENT and L.idkptGetTemporalDevicePtr(ctx, q, C.byref(p), C.byref(n)) == INVALID_ARGUMENT
    for nbytes in (buf.nbytes - 16, buf.nbytes + 16, 0):
        assert L.idkptDownloadGeometry(ctx, 0, buf.ctypes.data, nbytes) == INVALID_ARGUMENT and L.idkptDownloadTemporal(ctx, 0, buf.ctypes.data, nbytes) == INVALID_ARGUMENT
    assert L.idkptDownloadGeometry(ctx, 0, None, buf.nbytes) == INVALID_ARGUMENT and L.idkptGetTemporalDevicePtr(ctx, 0, None, None) == INVALID_ARGUMENT
    assert unchanged()
    # n == 0: a frame that has begun and rendered nothing
    assert pt.BeginFrame() == 0
    assert c_reproject(pt, 0, 1, s) == INVALID_OPERATION and unchanged()
    pt.Dispose()
    # no geometry in either slot, no temporal image in the history slot
    pt = new_pt(scene, W, H)
    pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute()
    assert c_reproject(pt, 0, T.IDKPT_NO_HISTORY, s) == INVALID_OPERATION          # slot 0 without geometry
    pt.CaptureGeometry()
    pt.BeginFrame(); pt.Compute(); pt.CaptureGeometry()
    assert c_reproject(pt, 1, 0, s) == INVALID_OPERATION                            # the history slot has geometry and no temporal image
    pt.Reproject(0, T.IDKPT_NO_HISTORY)
    assert c_reproject(pt, 1, 0, s) == 0
    pt.Dispose()
    # a slot with a temporal image and a history slot without geometry cannot happen (a temporal image needs its geometry); a ring of 1 has no second slot
    one = new_pt(scene, W, H, ring=1)
    one.SetCamera(cam_a); one.Compute(); one.CaptureGeometry()
    assert c_reproject(one, 0, 0, s) == INVALID_ARGUMENT and c_reproject(one, 0, T.IDKPT_NO_HISTORY, s) == 0
    one.Dispose()
    # no size set, no scene; a two-member context and a row-band context
    from idkengine_amd import _lib
    from idkengine_amd.pathtracer import PathTracer
    L = _lib.load()
    raw = C.c_void_p()
    assert L.idkptCreate(1, (C.c_int32 * 1)(0), C.byref(raw)) == 0
    assert L.idkptCaptureGeometry(raw, -1) == INVALID_OPERATION and L.idkptReproject(raw, 0, T.IDKPT_NO_HISTORY, C.addressof(s)) == INVALID_OPERATION
    assert L.idkptDownloadTemporal(raw, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION and L.idkptUseTemporalAsDenoised(raw, -1) == INVALID_OPERATION
    assert L.idkptDestroy(raw) == 0
    bare = PathTracer(W, H)
    assert bare._L.idkptCaptureGeometry(bare._ctx, -1) == INVALID_OPERATION                              # no scene uploaded
    bare.Dispose()
    for kw in (dict(devices=[0, 0]), dict(row_modulo=2, row_remainder=1, row_band=8)):
        pt = PathTracer(W, H, **kw)
        pt.UploadScene(scene); pt.SetCamera(cam_a); pt.Compute()
        assert pt._L.idkptCaptureGeometry(pt._ctx, -1) == INVALID_OPERATION and c_reproject(pt, 0, T.IDKPT_NO_HISTORY, s) == INVALID_OPERATION
        assert pt._L.idkptUseTemporalAsDenoised(pt._ctx, -1) == INVALID_OPERATION and pt._L.idkptDownloadGeometry(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
        assert pt._L.idkptSetDenoiseInput(pt._ctx, T.IDKPT_DENOISE_INPUT_TEMPORAL) == INVALID_OPERATION and pt._L.idkptSetDenoiseInput(pt._ctx, T.IDKPT_DENOISE_INPUT_ACCUMULATED) == 0
        pt.Dispose()


# ---- lifetime
def test_the_images_survive_the_reset_and_go_with_the_size(scene):
    W, H = 64, 64
    pt = new_pt(scene, W, H)
    cam_a, cam_b = sequence(pt, W, H)
    kept = [(pt.DownloadGeometry(q), pt.DownloadTemporal(q)) for q in (0, 1)]
    pt.ResetAccumulation(); pt.set_max_batch(4); pt.SetPresentationSize(32, 32)
    assert pt.BeginFrame() == 0
    for q in (0, 1):
        assert R.same(pt.DownloadGeometry(q), kept[q][0]) and R.same(pt.DownloadTemporal(q), kept[q][1])
    # surviving the reset is the point: the next frame reprojects onto the kept history
    pt.SetCamera(cam_b); pt.Compute(); pt.CaptureGeometry()
    pt.Reproject(0, 1, settings_for(cam_b))
    assert (pt.DownloadTemporal(0)[..., 3] > 1.0).mean() > 0.5
    assert guards_intact(pt, (0, 1))

    def gone():
        buf = np.zeros((pt.height, pt.width, 4), np.float32); p = C.c_void_p(); n = C.c_size_t()
        for q in (0, 1):
            assert pt._L.idkptDownloadGeometry(pt._ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
            assert pt._L.idkptDownloadTemporal(pt._ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
            assert pt._L.idkptGetGeometryDevicePtr(pt._ctx, q, C.byref(p), C.byref(n)) == INVALID_OPERATION
            assert pt._L.idkptGetTemporalDevicePtr(pt._ctx, q, C.byref(p), C.byref(n)) == INVALID_OPERATION
            assert pt._L.idkptUseTemporalAsDenoised(pt._ctx, q) == INVALID_OPERATION

    def again():
        pt.SetCamera(cam_a); pt.Compute(); pt.CaptureGeometry(); pt.Reproject(None, T.IDKPT_NO_HISTORY)
        assert guards_intact(pt, (0,))

    pt.SetSize(W, H); gone(); again()
    pt.SetFrameRing(3); gone(); again()
    for call in (lambda: pt._L.idkptSetRowSharding(pt._ctx, 1, 0), lambda: pt._L.idkptSetRowBands(pt._ctx, 8, 1, 0), lambda: pt._L.idkptSetRowRange(pt._ctx, 0, H)):
        assert call() == 0
        gone(); again()
    pt.SetSize(48, H); gone()                            # (another width; the strip set above still fits the height)
    pt.Dispose()
