"""History reconstruction on the device: idkptReconstructHistory (csrc/kernels_reconstruct.hpp k_reconstruct; the contract: include/idkpt.h, "history reconstruction").
Everything is bit for bit: the reconstructed temporal image against tests/reconstruct_ref.py (the numpy restatement of the header's text) applied to a snapshot of the
INPUT — the kernel works in place, so this is also the test of the header's in-place argument — and everything the call must not touch against what it was, or against
a context that never made the call.  The 64 guard bytes behind every image of the slot are looked at after every call.

The slots are real captures of the small Cornell box; the synthetic cases then overwrite the temporal and geometry images, Albedo and Normal through their device
pointers with a torch copy on the context's stream, as tests/test_gpu_denoise_temporal.py plants its images."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import reconstruct_ref as R  # noqa: E402
import denoise_temporal_ref as DT  # noqa: E402
from test_gpu_reproject import CAM_A, CAMS_B, SKY, settings_for  # noqa: E402
from test_gpu_denoise_temporal import new_pt, frame, write_ptr  # noqa: E402
from test_gpu_rectify import body_and_guard  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
NO_HISTORY = T.IDKPT_NO_HISTORY
FAST = dict(PositionTolerance=0.02, MaxHistory=4.0)


@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, sky_color=SKY)


def started(sc, w, h, **kw):
    """a context whose slot 0 holds a geometry image, a temporal image, a temporal moments image and a fast temporal image: what the planted cases overwrite"""
    pt = new_pt(sc, w, h, **kw)
    assert frame(pt, S.Camera(w, h, **CAM_A), 1) == 0
    pt.Reproject(0, NO_HISTORY); pt.ReprojectMoments(0, NO_HISTORY); pt.ReprojectFast(0, NO_HISTORY)
    return pt


def c_reconstruct(pt, s, slot=-1):
    d = s if isinstance(s, T.Reconstruct) else T.Reconstruct(**s)
    return pt._L.idkptReconstructHistory(pt._ctx, slot, C.addressof(d))


def slot_images(pt, slot):
    """{name: body} of every image of the slot, the temporal ones through their device pointers with their guards checked, each body equal to its download"""
    pairs = {"geometry": (pt.geometry_device_ptr, pt.DownloadGeometry), "temporal": (pt.temporal_device_ptr, pt.DownloadTemporal),
             "fast": (pt.fast_temporal_device_ptr, pt.DownloadFastTemporal), "moments": (pt.temporal_moments_device_ptr, pt.DownloadTemporalMoments)}
    out = {}
    for name, (ptr_fn, download) in pairs.items():
        body, guard = body_and_guard(pt, ptr_fn(slot))
        assert R.same(body, download(slot)), name
        assert (guard == 0xA5).all(), name
        out[name] = body.copy()
    for i, name in enumerate(("result", "albedo", "normal")):
        out[name] = pt.FrameResult(slot, i)
    out["luminance_moments"] = pt.DownloadMoments(slot)
    return out


UNTOUCHED = ("geometry", "fast", "moments", "result", "albedo", "normal", "luminance_moments")


def plant(pt, slot, t, g, a, n):
    write_ptr(pt, pt.temporal_device_ptr(slot), t); write_ptr(pt, pt.geometry_device_ptr(slot), g)
    write_ptr(pt, pt.frame_device_ptr(slot, 1), a); write_ptr(pt, pt.frame_device_ptr(slot, 2), n)


def differing(got, want):
    return int((R.bits(got) != R.bits(want)).any(axis=2).sum())


def reconstructed(pt, slot, s):
    """one idkptReconstructHistory held to the restatement on a snapshot of its input: returns (the slot's images after it, the restatement's stats)"""
    before = slot_images(pt, slot)
    ptr = pt.temporal_device_ptr(slot)
    st = {}
    want = R.reconstruct(before["temporal"], before["geometry"], before["albedo"], before["normal"], stats=st, **s)
    pt._check(c_reconstruct(pt, s, slot))
    assert pt.temporal_device_ptr(slot) == ptr                                 # in place: no swap
    after = slot_images(pt, slot)
    t, got = before["temporal"], after["temporal"]
    assert R.same(got, want), (s, differing(got, want))
    assert (R.bits(got[..., 3]) == R.bits(t[..., 3])).all()                      # the alpha plane
    with np.errstate(invalid="ignore"):
        keeps = (t[..., 3] >= F(s["FillBelow"])) | (R.bits(before["geometry"][..., 3]) == R.MISS_ID)
    assert R.same(got[keeps], t[keeps])
    for name in UNTOUCHED:
        assert R.same(after[name], before[name]), name
    return after, st


# ---- 1. the kernel, bit for bit, on planted images
@pytest.mark.parametrize("size", [(37, 23), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reconstruction_equals_the_restatement_of_the_input_snapshot_bit_for_bit(scene, size):
    W, H = size
    pt = started(scene, W, H)
    clean = R.random_images(W, H, seed=100 * W + H)
    branches = set()
    for name, (t, g, a, n) in (("clean", clean), ("planted", R.planted(*clean, seed=W + H))):
        for radius in (1, 2, 3):
            for stride in (1, 3, 8):
                s = dict(R.DEFAULTS, Radius=radius, Stride=stride)
                plant(pt, 0, t, g, a, n)
                after, st = reconstructed(pt, 0, s)
                assert st["written"].any() and R.same(after["geometry"], g) and R.same(after["albedo"], a) and R.same(after["normal"], n), (name, s)
                branches |= set(np.unique(st["branch"]).tolist())
    assert branches == {R.BRANCH_KEPT, R.BRANCH_NO_TAPS, R.BRANCH_WRITTEN, R.BRANCH_NOT_FINITE}
    assert pt.AccumulatedSamples == 1
    pt.Dispose()


def test_every_short_pixel_beside_every_long_one_across_tiles(scene):
    """a checkerboard of short and long pixels over 4 x 4 tiles, one surface: every written pixel's taps are pixels that are read only, its neighbours at odd offsets
    are written by other threads and other workgroups meanwhile — the result is the restatement's of the input whatever the order"""
    W = H = 64
    pt = started(scene, W, H)
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[0:H, 0:W]
    t = np.empty((H, W, 4), F); t[..., :3] = rng.random((H, W, 3)) * 2.0; t[..., 3] = np.where((xs + ys) % 2 == 0, 1.0, 9.0)
    g = np.zeros((H, W, 4), F); g[..., 3] = R.asfloat(np.uint32([3]))[0]
    a = np.ones((H, W, 4), F); a[..., :3] = (0.4 + 0.2 * rng.random((H, W, 3))).astype(F)
    n = np.ones((H, W, 4), F); n[..., :3] = F([0.0, 0.0, 1.0])
    for stride in (1, 2):                                 # stride 1: half of the 24 taps give; stride 2: every tap is a short pixel, nobody gives
        plant(pt, 0, t, g, a, n)
        after, st = reconstructed(pt, 0, dict(R.DEFAULTS, Stride=stride))
        short = t[..., 3] == 1.0
        assert (st["written"][short].all() if stride == 1 else not st["written"].any()) and not st["written"][~short].any()
    # a second call on its own output: the counts did not move, so the same pixels are filled again, from the same neighbours
    plant(pt, 0, t, g, a, n)
    first, _ = reconstructed(pt, 0, dict(R.DEFAULTS, Stride=1))
    second, st = reconstructed(pt, 0, dict(R.DEFAULTS, Stride=1))
    assert st["written"].sum() == W * H // 2 and not R.same(second["temporal"], first["temporal"])
    pt.Dispose()


# ---- 2. a real sequence: six one-sample frames under one camera, then a camera move that disoccludes
def sequence(sc, W, H, versions, reconstruct):
    pt = new_pt(sc, W, H)
    pt.SetSceneVersions(versions)
    cam_a, cam_b = S.Camera(W, H, **CAM_A), S.Camera(W, H, **CAMS_B["translation+yaw"])
    prev, prev_cam = NO_HISTORY, None
    out = {}
    for k in range(7):
        cam = cam_a if k < 6 else cam_b
        pt.SetSampleSequence(k, 1)                        # frame k draws sample k's random numbers: the static camera sees new noise every frame
        slot = frame(pt, cam, 1)
        s, sf = (T.Reproject(), T.Reproject(**FAST)) if prev_cam is None else (settings_for(prev_cam), settings_for(prev_cam, **FAST))
        pt.Reproject(slot, prev, s); pt.ReprojectMoments(slot, prev, s); pt.ReprojectFast(slot, prev, sf)
        if reconstruct:
            before = pt.DownloadTemporal(slot)
            after, st = reconstructed(pt, slot, dict(R.DEFAULTS))
            if k == 6:
                hit = R.bits(after["geometry"][..., 3]) != R.MISS_ID
                below = hit & (before[..., 3] < F(R.DEFAULTS["FillBelow"]))
                changed = (R.bits(after["temporal"]) != R.bits(before)).any(axis=2)
                print(f"scene versions {versions}: {int(hit.sum())} hit pixels, {int(below.sum())} below FillBelow, {int(changed.sum())} pixels changed")
                assert below.sum() >= 0.01 * hit.sum() and changed.sum() >= 1        # a condition on the input: the move disoccludes
                assert not changed[~below].any() and not changed[~st["written"]].any()   # (a written pixel may receive the bits it had: black stays black)
                out["denoised"] = pt.DenoiseTemporal(slot=slot)
                inputs = (after["temporal"], after["moments"], after["albedo"], after["normal"])
                want = DT.denoise_temporal(*inputs, **DT.DEFAULTS)
                assert R.same(out["denoised"], want), differing(out["denoised"], want)
        prev, prev_cam = slot, cam
    out.update(slot_images(pt, slot))
    out["samples"] = pt.AccumulatedSamples
    pt.Dispose()
    return out


def test_a_camera_move_that_disoccludes_and_nothing_else_notices(scene):
    W = H = 64
    one, two, never = sequence(scene, W, H, 1, True), sequence(scene, W, H, 2, True), sequence(scene, W, H, 1, False)
    for k in one:
        if k != "samples":
            assert R.same(one[k], two[k]), k                                   # one and two scene versions: the same bits
    for k in UNTOUCHED:
        assert R.same(one[k], never[k]), k                                     # what the call does not write is what a context that never called it holds
    assert one["samples"] == two["samples"] == never["samples"] == 1
    assert R.same(one["temporal"][..., 3], never["temporal"][..., 3]) and not R.same(one["temporal"], never["temporal"])


# ---- 3. the filter behind it
def test_denoise_temporal_reads_the_reconstructed_image(scene):
    W, H = 37, 29
    pt = started(scene, W, H)
    temporal, tm, albedo, normal = DT.random_images(W, H)
    g = pt.DownloadGeometry(0)
    write_ptr(pt, pt.temporal_moments_device_ptr(0), tm)
    plant(pt, 0, temporal, g, albedo, normal)
    after, st = reconstructed(pt, 0, dict(R.DEFAULTS, Stride=1))
    assert st["written"].sum() >= 0.05 * W * H and R.same(after["moments"], tm)
    for demod in (0, 1):
        s = DT.settings(3, demod)
        got = pt.DenoiseTemporal(T.DenoiseTemporal(**s), slot=0)
        want = DT.denoise_temporal(after["temporal"], tm, albedo, normal, **s)
        assert R.same(got, want), (demod, differing(got, want))
        assert not R.same(got, DT.denoise_temporal(temporal, tm, albedo, normal, **s))      # (the reconstruction reached the filter)
    pt.Dispose()


# ---- 4. refusals, in the documented order, each leaving the image's bits as they were
def test_refusals_in_order_and_the_no_op(scene):
    W, H = 37, 23
    pt = started(scene, W, H)
    t, g, a, n = R.random_images(W, H, seed=77)
    plant(pt, 0, t, g, a, n)
    before = slot_images(pt, 0)
    good = dict(R.DEFAULTS)

    def unchanged():
        now = slot_images(pt, 0)
        return all(R.same(now[k], before[k]) for k in before)

    nan, inf = float("nan"), float("inf")
    d = T.Reconstruct()
    L, ctx = pt._L, pt._ctx
    assert L.idkptReconstructHistory(ctx, 0, None) == INVALID_ARGUMENT and L.idkptReconstructHistory(None, 0, C.addressof(d)) == INVALID_ARGUMENT
    for slot in (-2, 2):
        assert L.idkptReconstructHistory(ctx, slot, C.addressof(d)) == INVALID_ARGUMENT
    bad = [dict(good, Radius=0), dict(good, Radius=4), dict(good, Radius=-1), dict(good, Stride=0), dict(good, Stride=9), dict(good, Stride=-3)]
    for key in ("FillBelow", "AlbedoSigma", "NormalSigma"):
        bad += [dict(good, **{key: v}) for v in (0.0, -1.0, nan, inf, -inf)]
    for s in bad:
        assert c_reconstruct(pt, s, 0) == INVALID_ARGUMENT, s
    # the order: the slot before the Radius, the Radius before the Stride, the Stride before FillBelow, FillBelow before the sigmas — told by the message
    def message(s, slot=0):
        assert c_reconstruct(pt, s, slot) == INVALID_ARGUMENT
        return last_error(pt)
    worst = dict(Radius=0, Stride=0, FillBelow=nan, AlbedoSigma=nan, NormalSigma=nan)
    assert "slot" in message(worst, 5) and "Radius" in message(worst) and "Stride" in message(dict(worst, Radius=2))
    assert "FillBelow" in message(dict(worst, Radius=2, Stride=3)) and "Sigma" in message(dict(worst, Radius=2, Stride=3, FillBelow=4.0))
    assert unchanged()
    # an argument error comes before every INVALID_OPERATION: slot 1 holds nothing yet
    assert c_reconstruct(pt, dict(good, Radius=0), 1) == INVALID_ARGUMENT and c_reconstruct(pt, good, 1) == INVALID_OPERATION
    assert unchanged()
    # FillBelow below every count: a no-op, bit for bit
    assert t[..., 3].min() >= 1.0 and c_reconstruct(pt, dict(good, FillBelow=0.5), 0) == 0 and unchanged()
    assert c_reconstruct(pt, good, 0) == 0 and not unchanged()                  # (the accepted call does move the image)
    pt.Dispose()
    # OutputAOVs off, before the slot's images are asked for; then a slot without a geometry image, and one without a temporal image
    cam_a = S.Camera(W, H, **CAM_A)
    pt = new_pt(scene, W, H, aovs=False)
    pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute()
    assert c_reconstruct(pt, good, 0) == INVALID_OPERATION and "OutputAOVs" in last_error(pt)
    pt.CaptureGeometry(); pt.Reproject(0, NO_HISTORY)
    kept = pt.DownloadTemporal(0)
    assert c_reconstruct(pt, good, 0) == INVALID_OPERATION and "OutputAOVs" in last_error(pt) and R.same(pt.DownloadTemporal(0), kept)
    pt.Dispose()
    pt = new_pt(scene, W, H)
    pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute()
    assert c_reconstruct(pt, good, 0) == INVALID_OPERATION and "geometry image" in last_error(pt)
    pt.CaptureGeometry()
    assert c_reconstruct(pt, good, 0) == INVALID_OPERATION and "temporal image" in last_error(pt)
    pt.Reproject(0, NO_HISTORY)
    assert c_reconstruct(pt, good, 0) == 0                                       # neither a moments image nor a fast one is needed
    pt.Dispose()
    # no size set; a two-member context and a row-band context: the scope, before OutputAOVs
    from idkengine_amd import _lib
    from idkengine_amd.pathtracer import PathTracer
    L = _lib.load()
    raw = C.c_void_p()
    assert L.idkptCreate(1, (C.c_int32 * 1)(0), C.byref(raw)) == 0
    assert L.idkptReconstructHistory(raw, -1, C.addressof(d)) == INVALID_OPERATION
    bad_d = T.Reconstruct(Radius=0)
    assert L.idkptReconstructHistory(raw, -1, C.addressof(bad_d)) == INVALID_ARGUMENT
    assert L.idkptDestroy(raw) == 0
    for kw in (dict(devices=[0, 0]), dict(row_modulo=2, row_remainder=1, row_band=8)):
        pt = PathTracer(W, H, **kw)
        pt.UploadScene(scene); pt.SetCamera(cam_a); pt.Compute()
        assert pt._L.idkptReconstructHistory(pt._ctx, -1, C.addressof(d)) == INVALID_OPERATION
        pt.Dispose()


def last_error(pt):
    msg = C.c_char_p()
    pt._L.idkptGetLastError(pt._ctx, C.byref(msg))
    return (msg.value or b"").decode()
