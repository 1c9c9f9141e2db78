"""History rectification on the device: idkptReprojectFast and idkptRectifyHistory (csrc/kernels_rectify.hpp k_rectify, csrc/kernels_reproject.hpp on the fast image pair;
the contract: include/idkpt.h, "history rectification").  Everything is bit for bit: the rectified image against tests/rectify_ref.py (the numpy restatement of the
header's text), the fast image against tests/reproject_ref.py / tests/motion_ref.py and against idkptReproject's own image where the two contracts coincide, the
accumulated images against a context that made none of the new calls.  The 64 guard bytes behind every image of the slot and behind the spare image are looked at after
every call.

The slots are real captures of the small Cornell box; the synthetic cases then overwrite the temporal, fast temporal, geometry and temporal moments images through their
device pointers with a torch copy on the context's stream, as tests/test_gpu_denoise_temporal.py plants its images."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import rectify_ref as R  # noqa: E402
import reproject_ref as P  # noqa: E402
import motion_ref as MR  # noqa: E402
from test_gpu_present import read_device  # noqa: E402
from test_gpu_reproject import CAM_A, CAMS_B, SKY, GUARD, settings_for  # noqa: E402
from test_gpu_denoise_temporal import new_pt, frame, write_ptr  # noqa: E402
from test_gpu_motion import new_pt as moving_pt, move_short_box, SHORT, CAM as CAM_FRONT  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
NO_HISTORY = T.IDKPT_NO_HISTORY
FAST = dict(PositionTolerance=0.02, MaxHistory=4.0)                          # the documented starting value of the fast cap


@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, sky_color=SKY)


@pytest.fixture(scope="module")
def moving_scene(native_builder):
    return S.cornell_scene(native_builder, instanced=True, sky_color=SKY, refittable=True)


def started(sc, w, h, moments=True, **kw):
    """a context whose slot 0 holds a geometry image, a temporal image, a fast temporal image and (moments) a temporal moments image: what the planted cases overwrite"""
    pt = new_pt(sc, w, h, noise=moments, **kw)
    assert frame(pt, S.Camera(w, h, **CAM_A), 1) == 0
    pt.Reproject(0, NO_HISTORY); pt.ReprojectFast(0, NO_HISTORY)
    if moments:
        pt.ReprojectMoments(0, NO_HISTORY)
    return pt


def c_rectify(pt, s, slot=-1):
    d = s if isinstance(s, T.Rectify) else T.Rectify(**s)
    return pt._L.idkptRectifyHistory(pt._ctx, slot, C.addressof(d))


def c_reproject_fast(pt, slot, history, s):
    return pt._L.idkptReprojectFast(pt._ctx, slot, history, C.addressof(s))


def body_and_guard(pt, ptr_and_bytes):
    p, n = ptr_and_bytes
    assert n == pt.height * pt.width * 16
    raw = read_device(pt, p, n + GUARD)
    return raw[:n].view(F).reshape(pt.height, pt.width, 4), raw[n:]


def images_of(pt, slot, moments):
    """{name: (body, guard)} of every image the slot holds, through the device pointers; each body equals its download"""
    pairs = {"geometry": (pt.geometry_device_ptr, pt.DownloadGeometry), "temporal": (pt.temporal_device_ptr, pt.DownloadTemporal), "fast": (pt.fast_temporal_device_ptr, pt.DownloadFastTemporal)}
    if moments:
        pairs["moments"] = (pt.temporal_moments_device_ptr, pt.DownloadTemporalMoments)
    out = {}
    for name, (ptr_fn, download) in pairs.items():
        body, guard = body_and_guard(pt, ptr_fn(slot))
        assert R.same(body, download(slot)), name
        assert (guard == 0xA5).all(), name
        out[name] = body
    return out


def plant(pt, slot, t, f, g, moments=None):
    write_ptr(pt, pt.temporal_device_ptr(slot), t); write_ptr(pt, pt.fast_temporal_device_ptr(slot), f); write_ptr(pt, pt.geometry_device_ptr(slot), g)
    if moments is not None:
        write_ptr(pt, pt.temporal_moments_device_ptr(slot), moments)


def rectified(pt, slot, s, moments):
    """one idkptRectifyHistory: returns the slot's images after it; the buffer that held the temporal image before the call is the spare one after it — its guard is
    looked at as well, and (the kernel wrote the OTHER buffer) its payload still holds the previous temporal image"""
    old = pt.temporal_device_ptr(slot)
    before = body_and_guard(pt, old)[0].copy()
    pt._check(c_rectify(pt, s, slot))
    after = images_of(pt, slot, moments)
    assert pt.temporal_device_ptr(slot)[0] != old[0]
    spare, guard = body_and_guard(pt, old)
    assert (guard == 0xA5).all() and R.same(spare, before)
    return after


def differing(got, want):
    return int((R.bits(got) != R.bits(want)).any(axis=2).sum())


def random_moments(W, H, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random((H, W, 4)) * 2.0).astype(F); m[..., 2] = 0.0; m[..., 3] = rng.integers(8, 33, (H, W)).astype(F)
    return m


# ---- 1. the kernel, bit for bit
@pytest.mark.parametrize("with_moments", [True, False], ids=["moments", "no-moments"])
@pytest.mark.parametrize("size", [(37, 29), (64, 48), (16, 16), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rectify_equals_the_restatement_bit_for_bit(scene, size, with_moments):
    W, H = size
    pt = started(scene, W, H, moments=with_moments)
    result = [pt.FrameResult(0, i) for i in range(3)]
    clean = R.random_images(W, H, seed=100 * W + H)
    branches = set()
    for name, (t, f, g) in (("clean", clean), ("planted", R.planted(*clean, seed=W + H))):
        eq = R.same if name == "clean" else R.nan_same
        mom = random_moments(W, H, W) if with_moments else None
        for radius in (1, 2, 3):
            s = dict(R.DEFAULTS, Radius=radius)
            plant(pt, 0, t, f, g, mom)
            st = {}
            want = R.rectify(t, f, g, stats=st, **s)
            got = rectified(pt, 0, s, with_moments)
            assert eq(got["temporal"], want), (name, radius, differing(got["temporal"], want))
            assert R.same(got["temporal"][~st["blended"]], t[~st["blended"]])
            assert R.same(got["fast"], f) and R.same(got["geometry"], g)          # read, not written
            if with_moments:
                assert R.same(got["moments"], R.rectify_moments(mom, want, st["blended"])), (name, radius)
                assert R.same(got["moments"][..., 3][st["blended"]], got["temporal"][..., 3][st["blended"]])
            branches |= set(np.unique(st["branch"]).tolist())
    if (W, H) != (1, 1):
        assert branches >= {R.BRANCH_FEW, R.BRANCH_ZERO, R.BRANCH_RAMP, R.BRANCH_FULL, R.BRANCH_NOT_FINITE}
    for i in range(3):
        assert R.same(pt.FrameResult(0, i), result[i])                           # the accumulated images are not touched
    assert pt.AccumulatedSamples == 1
    pt.Dispose()


def test_reads_precede_writes_across_tiles(scene):
    """a frame of 4 x 3 tiles whose every pixel is replaced (lambda = 1): a kernel that wrote the image it reads would hand a neighbouring workgroup differences of zero"""
    W, H = 64, 48
    pt = started(scene, W, H)
    t, f, g = R.uniform_change(W, H, seed=9)
    mom = random_moments(W, H, 4)
    for radius in (1, 2, 3):
        s = dict(R.DEFAULTS, Radius=radius)
        plant(pt, 0, t, f, g, mom)
        st = {}
        want = R.rectify(t, f, g, stats=st, **s)
        assert (st["branch"] == R.BRANCH_FULL).all() and R.same(want, f)
        got = rectified(pt, 0, s, True)
        assert R.same(got["temporal"], want), (radius, differing(got["temporal"], want))
        assert R.same(got["moments"][..., 3], f[..., 3]) and R.same(got["moments"][..., :3], mom[..., :3])
    # ... and a second call on its own output: the histories agree now, nothing moves
    again = rectified(pt, 0, s, True)
    assert R.same(again["temporal"], f) and R.same(again["moments"], got["moments"])
    pt.Dispose()


# ---- 2. the fast image
def test_reproject_fast_equals_the_restatement_and_reproject(scene):
    W, H = 64, 48
    pt = new_pt(scene, W, H, noise=False)
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["translation+yaw"])
    M = (cam_a.view @ cam_a.proj).astype(F)
    assert frame(pt, cam_a, 4) == 0
    pt.Reproject(0, NO_HISTORY); pt.ReprojectFast(0, NO_HISTORY)
    r0 = pt.FrameResult(0, 0)
    start = r0.copy(); start[..., 3] = 4.0
    assert R.same(pt.DownloadFastTemporal(0), start) and R.same(pt.DownloadTemporal(0), start)   # IDKPT_NO_HISTORY: (cur.rgb, n)
    assert frame(pt, cam_b, 2) == 1
    # histories that start equal, the same settings: the same image
    for s in (dict(P.DEFAULTS), FAST):
        pt.Reproject(1, 0, settings_for(cam_a, **s)); pt.ReprojectFast(1, 0, settings_for(cam_a, **s))
        assert R.same(pt.DownloadFastTemporal(1), pt.DownloadTemporal(1))
    # a fast history of its own: the restatement on the fast images
    rng = np.random.default_rng(31)
    hf = (rng.random((H, W, 4)) * 3.0).astype(F); hf[..., 3] = rng.integers(1, 9, (H, W)).astype(F)
    hf[H // 2, W // 2, 0] = np.nan; hf[H // 3, W // 2, 3] = np.inf
    hc = pt.DownloadTemporal(0)
    write_ptr(pt, pt.fast_temporal_device_ptr(0), hf)
    g0, g1, cur = pt.DownloadGeometry(0), pt.DownloadGeometry(1), pt.FrameResult(1, 0)
    t1 = pt.DownloadTemporal(1)
    pt.ReprojectFast(1, 0, settings_for(cam_a, **FAST))
    st = {}
    want = P.reproject(cur, 2, g1, g0, hf, M, cam_a.position, stats=st, **FAST)
    got = images_of(pt, 1, False)
    assert R.same(got["fast"], want), differing(got["fast"], want)
    assert st["history"].mean() > 0.3 and (~st["history"]).any() and (want[..., 3] <= 6.0).all() and (want[..., 3] == 6.0).any()      # the cap at 4, n = 2
    assert R.same(got["temporal"], t1) and R.same(pt.DownloadTemporal(0), hc) and R.same(pt.DownloadFastTemporal(0), hf)              # neither call touches the other's images
    images_of(pt, 0, False)
    pt.Dispose()


def test_reproject_fast_through_a_motion_image(moving_scene):
    W, H = 70, 37
    cam = S.Camera(W, H, **CAM_FRONT)
    M = (cam.view @ cam.proj).astype(F)
    pt = moving_pt(moving_scene, W, H)
    assert pt.BeginFrame() == 0
    pt.SetCamera(cam)
    for _ in range(4):
        pt.Compute()
    pt.CaptureMotion(); pt.Reproject(0, NO_HISTORY); pt.ReprojectFast(0, NO_HISTORY)
    move_short_box(pt, moving_scene)
    assert pt.BeginFrame() == 1
    pt.Compute()
    pt.CaptureMotion()
    sa = settings_for(cam, **FAST)
    pt.Reproject(1, 0, sa); pt.ReprojectFast(1, 0, sa)
    fast = pt.DownloadFastTemporal(1)
    assert R.same(fast, pt.DownloadTemporal(1))
    g, l, hg, hf, cur = pt.DownloadGeometry(1), pt.DownloadMotion(1), pt.DownloadGeometry(0), pt.DownloadFastTemporal(0), pt.FrameResult(1, 0)
    st = {}
    want = MR.reproject(cur, 1, g, l, hg, hf, M, cam.position, stats=st, **FAST)
    box = R.bits(g[..., 3]) == SHORT
    assert box.mean() >= 0.02 and st["history"][box].mean() >= 0.5            # the mover found its history through the motion image
    assert R.same(fast, want), differing(fast, want)
    assert (body_and_guard(pt, pt.fast_temporal_device_ptr(1))[1] == 0xA5).all() and (body_and_guard(pt, pt.motion_device_ptr(1))[1] == 0xA5).all()
    pt.Dispose()


# ---- 3. life cycle
def test_the_fast_image_survives_what_the_temporal_image_survives(scene):
    W, H = 64, 48
    pt = new_pt(scene, W, H)
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["translation+yaw"])
    frame(pt, cam_a, 2); pt.Reproject(0, NO_HISTORY); pt.ReprojectFast(0, NO_HISTORY); pt.ReprojectMoments(0, NO_HISTORY)
    frame(pt, cam_b, 1); pt.Reproject(1, 0, settings_for(cam_a)); pt.ReprojectFast(1, 0, settings_for(cam_a, **FAST)); pt.ReprojectMoments(1, 0, settings_for(cam_a))
    pt.RectifyHistory(slot=1)
    kept = [pt.DownloadFastTemporal(q) for q in (0, 1)]
    kept_t = [pt.DownloadTemporal(q) for q in (0, 1)]
    assert (kept[1][..., 3] > 1.0).mean() > 0.5
    pt.ResetAccumulation(); pt.set_max_batch(4); pt.SetPresentationSize(32, 32)
    assert pt.BeginFrame() == 0
    for q in (0, 1):
        assert R.same(pt.DownloadFastTemporal(q), kept[q]) and R.same(pt.DownloadTemporal(q), kept_t[q])
    pt.SetCamera(cam_b); pt.Compute(); pt.CaptureGeometry()                  # a capture does not drop it
    assert R.same(pt.DownloadFastTemporal(0), kept[0])
    # surviving is the point: the next frame reprojects onto the kept history and is rectified
    pt.Reproject(0, 1, settings_for(cam_b)); pt.ReprojectFast(0, 1, settings_for(cam_b, **FAST))
    assert (pt.DownloadFastTemporal(0)[..., 3] > 1.0).mean() > 0.5
    pt.RectifyHistory(slot=0)
    images_of(pt, 0, True); images_of(pt, 1, True)

    def gone():
        buf = np.zeros((pt.height, pt.width, 4), F); p = C.c_void_p(); n = C.c_size_t()
        for q in (0, 1):
            assert pt._L.idkptDownloadFastTemporal(pt._ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
            assert pt._L.idkptGetFastTemporalDevicePtr(pt._ctx, q, C.byref(p), C.byref(n)) == INVALID_OPERATION
            assert c_rectify(pt, R.DEFAULTS, q) == INVALID_OPERATION

    pt.SetSize(W, H); gone()
    pt.SetCamera(cam_a); pt.Compute(); pt.CaptureGeometry(); pt.Reproject(None, NO_HISTORY); pt.ReprojectFast(None, NO_HISTORY)
    pt.RectifyHistory()                                                       # (the spare image is made again after the resize)
    images_of(pt, None, False)
    pt.SetFrameRing(3); gone()
    pt.Dispose()


# ---- 4. refusals
def test_refusals_leave_the_previous_images_as_they_were(scene):
    W, H = 37, 29
    pt = started(scene, W, H)
    t, f, g = R.random_images(W, H, seed=77)
    mom = random_moments(W, H, 78)
    plant(pt, 0, t, f, g, mom)
    good = dict(R.DEFAULTS)

    def unchanged():
        im = images_of(pt, 0, True)
        return R.same(im["temporal"], t) and R.same(im["fast"], f) and R.same(im["moments"], mom) and R.same(im["geometry"], g)

    nan, inf = float("nan"), float("inf")
    bad = [dict(good, Radius=0), dict(good, Radius=4), dict(good, Radius=-1), dict(good, ZLow=0.0), dict(good, ZLow=-1.0), dict(good, ZLow=nan), dict(good, ZLow=inf),
           dict(good, ZHigh=3.0), dict(good, ZHigh=2.0), dict(good, ZHigh=nan), dict(good, ZHigh=inf), dict(good, Epsilon=0.0), dict(good, Epsilon=-1e-3), dict(good, Epsilon=nan), dict(good, Epsilon=inf)]
    for s in bad:
        assert c_rectify(pt, s, 0) == INVALID_ARGUMENT, s
    d = T.Rectify()
    for slot in (-2, 2):
        assert pt._L.idkptRectifyHistory(pt._ctx, slot, C.addressof(d)) == INVALID_ARGUMENT
    assert pt._L.idkptRectifyHistory(pt._ctx, 0, None) == INVALID_ARGUMENT and pt._L.idkptRectifyHistory(None, 0, C.addressof(d)) == INVALID_ARGUMENT
    assert unchanged()
    # idkptReprojectFast: idkptReproject's argument checks
    cam_a = S.Camera(W, H, **CAM_A)
    sa = settings_for(cam_a, **FAST)
    assert frame(pt, S.Camera(W, H, **CAMS_B["translation+yaw"]), 1) == 1
    for b in (dict(PositionTolerance=0.0), dict(PositionTolerance=nan), dict(PositionTolerance=inf), dict(MaxHistory=0.5), dict(MaxHistory=nan), dict(MaxHistory=inf)):
        assert c_reproject_fast(pt, 1, 0, settings_for(cam_a, **dict(FAST, **b))) == INVALID_ARGUMENT, b
    assert c_reproject_fast(pt, 1, 1, sa) == INVALID_ARGUMENT and c_reproject_fast(pt, -1, 1, sa) == INVALID_ARGUMENT      # slot == historySlot (-1 is slot 1 here)
    for slot, hist in ((2, 0), (-2, 0), (1, 2), (1, -1), (1, -3)):
        assert c_reproject_fast(pt, slot, hist, sa) == INVALID_ARGUMENT, (slot, hist)
    assert pt._L.idkptReprojectFast(pt._ctx, 1, 0, None) == INVALID_ARGUMENT
    buf = np.zeros((H, W, 4), F); p = C.c_void_p(); n = C.c_size_t()
    L, ctx = pt._L, pt._ctx
    for q in (-2, 2):
        assert L.idkptDownloadFastTemporal(ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_ARGUMENT and L.idkptGetFastTemporalDevicePtr(ctx, q, C.byref(p), C.byref(n)) == INVALID_ARGUMENT
    for nbytes in (buf.nbytes - 16, buf.nbytes + 16, 0):
        assert L.idkptDownloadFastTemporal(ctx, 0, buf.ctypes.data, nbytes) == INVALID_ARGUMENT
    assert L.idkptDownloadFastTemporal(ctx, 0, None, buf.nbytes) == INVALID_ARGUMENT and L.idkptGetFastTemporalDevicePtr(ctx, 0, None, None) == INVALID_ARGUMENT
    assert L.idkptDownloadFastTemporal(ctx, 1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION      # slot 1 holds none yet
    assert c_rectify(pt, good, 1) == INVALID_OPERATION                                                  # ... and no temporal image
    assert unchanged()
    # n == 0: a frame that has begun and rendered nothing
    assert c_reproject_fast(pt, 1, 0, sa) == 0
    kept = pt.DownloadFastTemporal(1)
    assert pt.BeginFrame() == 0
    assert c_reproject_fast(pt, 0, 1, sa) == INVALID_OPERATION and unchanged() and R.same(pt.DownloadFastTemporal(1), kept)
    assert c_rectify(pt, good, 0) == 0 and not R.same(pt.DownloadTemporal(0), t)                        # (the accepted call does move the image)
    pt.Dispose()
    # the slot without a geometry image, without a temporal image, without a fast temporal image; the history slot without a fast temporal image
    pt = new_pt(scene, W, H)
    pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute()
    assert c_rectify(pt, good, 0) == INVALID_OPERATION and c_reproject_fast(pt, 0, NO_HISTORY, sa) == INVALID_OPERATION
    pt.CaptureGeometry()
    assert c_rectify(pt, good, 0) == INVALID_OPERATION
    pt.Reproject(0, NO_HISTORY)
    assert c_rectify(pt, good, 0) == INVALID_OPERATION                       # a temporal image, no fast one
    pt.BeginFrame(); pt.Compute(); pt.CaptureGeometry()
    assert c_reproject_fast(pt, 1, 0, sa) == INVALID_OPERATION               # the history slot has geometry and a temporal image, no fast one
    pt.ReprojectFast(0, NO_HISTORY)
    assert c_rectify(pt, good, 0) == 0 and c_reproject_fast(pt, 1, 0, sa) == 0
    assert c_rectify(pt, good, 1) == INVALID_OPERATION                       # a fast image, no temporal one
    pt.Dispose()
    # no size set; a two-member context and a row-band context
    from idkengine_amd import _lib
    from idkengine_amd.pathtracer import PathTracer
    L = _lib.load()
    raw = C.c_void_p()
    assert L.idkptCreate(1, (C.c_int32 * 1)(0), C.byref(raw)) == 0
    assert L.idkptReprojectFast(raw, 0, NO_HISTORY, C.addressof(sa)) == INVALID_OPERATION and L.idkptRectifyHistory(raw, -1, C.addressof(d)) == INVALID_OPERATION
    assert L.idkptDownloadFastTemporal(raw, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
    assert L.idkptDestroy(raw) == 0
    for kw in (dict(devices=[0, 0]), dict(row_modulo=2, row_remainder=1, row_band=8)):
        pt = PathTracer(W, H, **kw)
        pt.UploadScene(scene); pt.SetCamera(cam_a); pt.Compute()
        assert c_reproject_fast(pt, 0, NO_HISTORY, sa) == INVALID_OPERATION and pt._L.idkptRectifyHistory(pt._ctx, -1, C.addressof(d)) == INVALID_OPERATION
        assert pt._L.idkptDownloadFastTemporal(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
        pt.Dispose()


# ---- 5. end to end: eight one-sample frames, the light four times as bright, eight more
def test_sixteen_frames_around_a_lighting_change_and_nothing_else_notices(scene):
    W, H = 64, 48
    cam = S.Camera(W, H, **CAM_FRONT)
    long_s, fast_s = settings_for(cam), settings_for(cam, **FAST)
    new, old = new_pt(scene, W, H), new_pt(scene, W, H)
    assert (scene.materials["EmissiveFactor"].max(axis=1) > 0).any()
    prev = NO_HISTORY
    touched = []
    for k in range(16):
        if k == 8:
            brighter = scene.materials.copy(); brighter["EmissiveFactor"] *= F(4.0)
            for pt in (new, old):
                pt.UpdateBuffer(T.IDKPT_BUF_MATERIALS, brighter)
        for pt in (new, old):
            pt.SetSampleSequence(k, 1)                                            # frame k draws sample k's random numbers: the static camera sees new noise every frame
            slot = frame(pt, cam, 1)
        new.Reproject(slot, prev, long_s); new.ReprojectMoments(slot, prev, long_s); new.ReprojectFast(slot, prev, fast_s)
        t, f, g, mom = new.DownloadTemporal(slot), new.DownloadFastTemporal(slot), new.DownloadGeometry(slot), new.DownloadTemporalMoments(slot)
        assert R.same(mom[..., 3], t[..., 3]), k
        st = {}
        want = R.rectify(t, f, g, stats=st, **R.DEFAULTS)
        got = rectified(new, slot, R.DEFAULTS, True)
        assert R.same(got["temporal"], want), (k, differing(got["temporal"], want))
        assert R.same(got["moments"], R.rectify_moments(mom, want, st["blended"])) and R.same(got["moments"][..., 3], got["temporal"][..., 3]), k
        assert R.same(got["fast"], f) and R.same(got["geometry"], g), k
        new.DenoiseTemporal(slot=slot)                                          # the filter takes the fractional counts
        touched.append(int(st["blended"].sum()))
        # everything the old calls make is what it is without the new ones
        for image in range(3):
            assert R.same(new.FrameResult(slot, image), old.FrameResult(slot, image)), (k, image)
        assert new.AccumulatedSamples == old.AccumulatedSamples == 1
        prev = slot
    assert max(touched[8:]) > 0, touched                                         # after the change some pixel has lambda > 0
    assert (got["fast"][..., 3] <= 5.0).all() and got["temporal"][..., 3].max() > 5.0
    new.Dispose(); old.Dispose()
