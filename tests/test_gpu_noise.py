"""The noise estimate on the device: the luminance moments k_final_draw_noise folds while idkptSetNoiseEstimate is on, and idkptEstimateNoise's tile map and summary
(csrc/kernels_noise.hpp), bit for bit against tests/noise_ref.py (the numpy restatement of the header's text).

Per-sample ground truth comes from paths the suite already verifies: for k = 0..5 a context with the switch OFF renders ONE sample of idkptSetSampleSequence(k, 1) into
freshly zeroed images; its weight is 1, so the downloaded Result is sample k's folded value nr exactly (0 * (1 - 1) + nr * 1).  The default sequence's sample k has the same
index (first + accumulated * stride), so the restatement folded over those six images is what the moments must hold after n samples — whatever the batch size, the ring
slot or OutputAOVs.  Scene: the 32-triangle Cornell box under a constant sky, seen from outside so that tiles pre-classified as sky (classes 1 - 6) and tiles on the
per-pixel path (class 0) both occur (asserted where the first-hit stage classifies at all: OutputAOVs 0); 24 x 16 (whole tiles) and 20 x 13 (tiles cut at the right and the bottom edge); RayDepth 3."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import noise_ref as R  # noqa: E402
from test_gpu_present import read_device  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
GUARD = 64
SAMPLES = 6
SIZES = [(24, 16), (20, 13)]
SKY = (0.4, 0.6, 0.9)


def camera(w, h):
    # the box in the middle of the frame; the tile columns beside it see sky only, by more than the classifier's margin of one pixel, and the field of view is narrow
    # enough that the pyramid of a tile cut by the image's edge (which reaches 8 pixels past it) still looks at one face of the sky
    return S.Camera(w, h, position=(0.0, 0.0, 11.0), fovy_deg=40.0)


def new_pt(sc, w, h, noise=False, aovs=0, max_batch=None, ring=None, debug=False, **kw):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h, **kw)
    pt.UploadScene(sc); pt.SetCamera(camera(w, h)); pt.RayDepth = 3
    if aovs:
        pt.OutputAOVs = 1
    if debug:
        pt.DoDebugBVHTraversal = True
    if max_batch is not None:
        pt.set_max_batch(max_batch)
    if ring is not None:
        pt.SetFrameRing(ring)
    if noise:
        pt.SetNoiseEstimate(True)
    return pt


@pytest.fixture(scope="module")
def clean_scene(native_builder):
    return S.cornell_scene(native_builder, variant="diffuse", sky_color=SKY)


@pytest.fixture(scope="module")
def planted_scene(native_builder):
    """the same box with an emissive factor of +Inf on its light: every path that reaches the light carries a non-finite radiance"""
    sc = S.cornell_scene(native_builder, variant="diffuse", sky_color=SKY)
    lit = np.flatnonzero((sc.materials["EmissiveFactor"] != 0).any(axis=1))
    assert len(lit) == 1
    sc.materials["EmissiveFactor"][lit[0]] = np.inf
    return sc


_TRUTH = {}


def truth(sc, key, w, h, debug=False):
    """the six per-sample images nr (computed once per scene, size and mode, shared and never written)"""
    k = (key, w, h, debug)
    if k not in _TRUTH:
        pt = new_pt(sc, w, h, debug=debug)
        out = []
        for i in range(SAMPLES):
            pt.SetSize(w, h)                              # zeroed images: the one sample below is folded onto 0 with weight 1
            pt.SetSampleSequence(i, 1)
            pt.Compute()
            assert pt.AccumulatedSamples == 1
            img = pt.Result; img.setflags(write=False)
            out.append(img)
        pt.Dispose()
        _TRUTH[k] = out
    return _TRUTH[k]


def moments_and_guard(pt, slot=None):
    """(the moments image through the device pointer, its guard bytes); the download must agree"""
    p, n = pt.moments_device_ptr(slot)
    assert n == pt.height * pt.width * 16
    raw = read_device(pt, p, n + GUARD)
    body = raw[:n].view(F).reshape(pt.height, pt.width, 4)
    down = pt.DownloadMoments(slot)
    assert (R.bits(body) == R.bits(down)).all()
    return down, raw[n:]


def noise_and_guards(pt, slot=None):
    """(tiles, summary) of the slot's estimate through the download, compared with the device pointers; asserts the guard bytes of both buffers"""
    tiles, s = pt.DownloadNoise(slot)
    pt_tiles, pt_sum, nbytes = pt.noise_device_ptrs(slot)
    assert nbytes == tiles.nbytes
    raw = read_device(pt, pt_tiles, nbytes + GUARD)
    assert (raw[:nbytes].view(np.uint32) == R.bits(tiles).reshape(-1)).all() and (raw[nbytes:] == 0xA5).all()
    raws = read_device(pt, pt_sum, 16 + GUARD)
    w = raws[:16].view(np.uint32)
    assert (int(w[0]), int(w[2]), int(w[3])) == (s["TilesAbove"], s["Tiles"], s["Samples"]) and w[1:2].view(F)[0].tobytes() == F(s["MaxTileMean"]).tobytes()
    assert (raws[16:] == 0xA5).all()
    return tiles, s


def c_estimate(pt, eps=1e-2, thr=0.05, slot=-1):
    p = T.Noise(eps, thr)
    return pt._L.idkptEstimateNoise(pt._ctx, slot, C.addressof(p))


def two_thresholds(m1, m2, n):
    """two thresholds between distinct tile means of the restatement, so that TilesAbove is neither 0 nor every tile"""
    means = np.unique(R.estimate(m1, m2, n)[0][..., 0])
    assert len(means) >= 3 and np.isfinite(means).all(), means
    return [float((float(means[0]) + float(means[1])) / 2), float((float(means[-2]) + float(means[-1])) / 2)]


def check_estimates(pt, m1, m2, n, slot=None):
    before = [pt.FrameResult(0 if slot is None else slot, i) for i in range(3)]
    for thr in two_thresholds(m1, m2, n):
        want_tiles, want_s = R.estimate(m1, m2, n, 1e-2, thr)
        assert 0 < want_s["TilesAbove"] < want_s["Tiles"]
        pt._check(c_estimate(pt, 1e-2, thr, -1 if slot is None else slot))
        tiles, s = noise_and_guards(pt, slot)
        print(f"[noise] {pt.width} x {pt.height}, n = {n}, threshold {thr:.4g}: {s}")
        assert R.same(tiles, want_tiles), int((R.bits(tiles) != R.bits(want_tiles)).sum())
        assert R.same_summary(s, want_s), (s, want_s)
    mom, guard = moments_and_guard(pt, slot)
    assert R.same(mom, R.moments_image(m1, m2)) and (guard == 0xA5).all()   # the estimate reads the moments and changes nothing
    for i in range(3):
        assert R.same(pt.FrameResult(0 if slot is None else slot, i), before[i])


CASES = {
    "24x16-batch1-aovs0": dict(size=(24, 16), max_batch=1, aovs=0),
    "24x16-batch4-aovs1": dict(size=(24, 16), max_batch=4, aovs=1),
    "20x13-batch4-aovs0": dict(size=(20, 13), max_batch=4, aovs=0),
    "20x13-batch1-aovs1": dict(size=(20, 13), max_batch=1, aovs=1),
    "24x16-batch4-debug": dict(size=(24, 16), max_batch=4, aovs=0, debug=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_moments_tiles_and_summary_equal_the_restatement_and_the_images_do_not_change(clean_scene, name):
    case = CASES[name]; (w, h) = case["size"]; debug = case.get("debug", False)
    nr = truth(clean_scene, "clean", w, h, debug)
    on = new_pt(clean_scene, w, h, noise=True, aovs=case["aovs"], max_batch=case["max_batch"], debug=debug)
    off = new_pt(clean_scene, w, h, noise=False, aovs=case["aovs"], max_batch=case["max_batch"], debug=debug)
    assert on.GetNoiseEstimate() and not off.GetNoiseEstimate()
    for n in range(1, SAMPLES + 1):
        on.Compute(); off.Compute()
        if n in (2, 6):                                   # with idkptSetMaxBatch(4): a batch of 2 the download launches, then samples 2..5 as one full batch
            m1, m2 = R.moments(nr[:n])
            mom, guard = moments_and_guard(on)
            assert R.same(mom, R.moments_image(m1, m2)), (n, int((R.bits(mom) != R.bits(R.moments_image(m1, m2))).any(axis=2).sum()))
            assert (guard == 0xA5).all()
            for i in range(3):                            # Result, Albedo, Normal: bit for bit what the switch-off context holds
                assert R.same(on.FrameResult(0, i), off.FrameResult(0, i)), (n, i)
    assert on.AccumulatedSamples == SAMPLES
    if not debug and not case["aovs"]:                    # (with OutputAOVs, and in the debug mode, the first-hit stage classifies no tile: every pixel takes the cls == 0 path)
        cls = on.tile_classes()
        assert cls.shape[0] >= 1 and ((cls >= 1) & (cls <= 6)).any() and (cls == 0).any(), cls   # pre-classified sky tiles and the per-pixel path both occurred
    check_estimates(on, *R.moments(nr), SAMPLES)
    on.Dispose(); off.Dispose()


def test_a_frame_that_begins_inside_a_batch_switches_the_moments_slot(clean_scene):
    w, h = 20, 13
    nr = truth(clean_scene, "clean", w, h)
    on = new_pt(clean_scene, w, h, noise=True, aovs=1, max_batch=4, ring=2)
    off = new_pt(clean_scene, w, h, noise=False, aovs=1, max_batch=4, ring=2)
    for pt in (on, off):
        assert pt.BeginFrame() == 0
        pt.Compute(); pt.Compute()
        assert pt.BeginFrame() == 1                       # inside the batch of 4: samples 2 and 3 of the batch belong to slot 1
        pt.Compute(); pt.Compute(); pt.Compute()
    for slot, n in ((0, 2), (1, 3)):
        m1, m2 = R.moments(nr[:n])                        # (a new frame restarts at sample index 0)
        mom, guard = moments_and_guard(on, slot)
        assert R.same(mom, R.moments_image(m1, m2)), slot
        assert (guard == 0xA5).all()
        for i in range(3):
            assert R.same(on.FrameResult(slot, i), off.FrameResult(slot, i)), (slot, i)
        check_estimates(on, m1, m2, n, slot)
    on.Dispose(); off.Dispose()


def test_a_planted_non_finite_radiance_makes_its_tiles_infinite_and_no_other(clean_scene, planted_scene):
    w, h = 24, 16
    nr = truth(planted_scene, "planted", w, h)
    m1, m2 = R.moments(nr)
    bad = ~(np.isfinite(m1) & np.isfinite(m2))
    assert bad.any() and not bad.all()
    pt = new_pt(planted_scene, w, h, noise=True, max_batch=4)
    for _ in range(SAMPLES):
        pt.Compute()
    mom, guard = moments_and_guard(pt)
    want = R.moments_image(m1, m2)
    both_nan = np.isnan(mom) & np.isnan(want)                                # a NaN's payload is the processor's own; everything else bit for bit
    assert ((R.bits(mom) == R.bits(want)) | both_nan).all() and (guard == 0xA5).all()
    pt._check(c_estimate(pt))
    tiles, s = noise_and_guards(pt)
    want_tiles, want_s = R.estimate(m1, m2, SAMPLES)
    assert R.same(tiles, want_tiles) and R.same_summary(s, want_s)
    bad_tiles = np.zeros(tiles.shape[:2], bool)
    for y, x in np.argwhere(bad):
        bad_tiles[y // 8, x // 8] = True
    assert bad_tiles.any() and not bad_tiles.all()
    assert np.isposinf(tiles[bad_tiles]).all() and np.isposinf(s["MaxTileMean"])          # e = +Inf: the tile's max and, through the tree, its mean
    clean_tiles, _ = R.estimate(*R.moments(truth(clean_scene, "clean", w, h)), SAMPLES)
    assert R.same(tiles[~bad_tiles], clean_tiles[~bad_tiles])                            # no other tile changes: the samples that never reach the light are the clean scene's
    pt.Dispose()


def test_toggling_restarts_the_accumulation_and_off_is_todays_library(clean_scene):
    w, h = 20, 13
    nr = truth(clean_scene, "clean", w, h)
    pt = new_pt(clean_scene, w, h, max_batch=4)
    pt.Compute(); pt.Compute(); pt.Compute()
    assert pt.AccumulatedSamples == 3
    pt.SetNoiseEstimate(False)                            # the value it has: nothing happens
    assert pt.AccumulatedSamples == 3
    pt.SetNoiseEstimate(True)
    assert pt.GetNoiseEstimate() and pt.AccumulatedSamples == 0
    mom, guard = moments_and_guard(pt)
    assert not mom.any() and (guard == 0xA5).all()        # zeroed at first use
    pt.Compute(); pt.Compute()
    m1, m2 = R.moments(nr[:2])
    assert R.same(pt.DownloadMoments(), R.moments_image(m1, m2))
    # kept by idkptSetMaxBatch (with the moments), idkptSetSize and idkptSetFrameRing (which re-make the images)
    pt.set_max_batch(2)
    assert pt.GetNoiseEstimate() and pt.AccumulatedSamples == 2 and R.same(pt.DownloadMoments(), R.moments_image(m1, m2))
    pt.Compute()
    assert R.same(pt.DownloadMoments(), R.moments_image(*R.moments(nr[:3])))
    pt.SetSize(w, h)
    assert pt.GetNoiseEstimate() and pt.AccumulatedSamples == 0 and not pt.DownloadMoments().any()
    pt.SetFrameRing(2)
    assert pt.GetNoiseEstimate()
    pt.SetFrameRing(1)
    pt.Compute(); pt.Compute()
    assert R.same(pt.DownloadMoments(), R.moments_image(m1, m2))
    pt.SetNoiseEstimate(False)
    assert not pt.GetNoiseEstimate() and pt.AccumulatedSamples == 0
    assert pt._L.idkptDownloadMoments(pt._ctx, -1, np.zeros(h * w * 4, F).ctypes.data, h * w * 16) == INVALID_OPERATION
    pt.Dispose()


def test_error_paths(clean_scene):
    w, h = 24, 16
    pt = new_pt(clean_scene, w, h)
    buf = np.zeros(h * w * 4, F); tiles = np.zeros(3 * 2 * 2, F); s = T.NoiseSummary()
    pt.Compute(); pt.Compute()
    # the switch is off
    assert c_estimate(pt) == INVALID_OPERATION
    assert pt._L.idkptDownloadMoments(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
    assert pt._L.idkptDownloadNoise(pt._ctx, -1, tiles.ctypes.data, tiles.nbytes, C.addressof(s)) == INVALID_OPERATION
    pt.SetNoiseEstimate(True)
    # fewer than two samples
    assert c_estimate(pt) == INVALID_OPERATION
    pt.Compute()
    assert c_estimate(pt) == INVALID_OPERATION
    pt.Compute()
    # a read before any estimate
    assert pt._L.idkptDownloadNoise(pt._ctx, -1, tiles.ctypes.data, tiles.nbytes, C.addressof(s)) == INVALID_OPERATION
    p = C.c_void_p()
    assert pt._L.idkptGetNoiseDevicePtr(pt._ctx, -1, C.byref(p), None, None) == INVALID_OPERATION
    # a bad slot, bad parameters: refused before anything is launched
    assert c_estimate(pt, slot=1) == INVALID_ARGUMENT and c_estimate(pt, slot=-2) == INVALID_ARGUMENT
    for eps in (0.0, -1.0, np.nan, np.inf):
        assert c_estimate(pt, eps=eps) == INVALID_ARGUMENT, eps
    for thr in (-1.0, np.nan, np.inf):
        assert c_estimate(pt, thr=thr) == INVALID_ARGUMENT, thr
    assert pt._L.idkptEstimateNoise(pt._ctx, -1, None) == INVALID_ARGUMENT
    assert pt._L.idkptSetNoiseEstimate(pt._ctx, 2) == INVALID_ARGUMENT
    assert pt._L.idkptDownloadNoise(pt._ctx, -1, tiles.ctypes.data, tiles.nbytes, C.addressof(s)) == INVALID_OPERATION   # none of those left an estimate
    assert c_estimate(pt, thr=0.0) == 0
    # wrong bytes, bad slots of the readbacks; either pointer of the download may be NULL
    assert pt._L.idkptDownloadNoise(pt._ctx, -1, tiles.ctypes.data, tiles.nbytes - 8, C.addressof(s)) == INVALID_ARGUMENT
    assert pt._L.idkptDownloadNoise(pt._ctx, 1, tiles.ctypes.data, tiles.nbytes, C.addressof(s)) == INVALID_ARGUMENT
    assert pt._L.idkptDownloadMoments(pt._ctx, -1, buf.ctypes.data, buf.nbytes - 16) == INVALID_ARGUMENT
    assert pt._L.idkptDownloadMoments(pt._ctx, 1, buf.ctypes.data, buf.nbytes) == INVALID_ARGUMENT
    assert pt._L.idkptDownloadNoise(pt._ctx, -1, None, 0, C.addressof(s)) == 0 and (s.Tiles, s.Samples) == (6, 2)
    assert pt._L.idkptDownloadNoise(pt._ctx, -1, tiles.ctypes.data, tiles.nbytes, None) == 0
    noise_and_guards(pt)
    assert pt.AccumulatedSamples == 2                      # nothing above touched the accumulation
    # a resize drops the estimate
    pt.SetSize(w, h)
    assert pt._L.idkptDownloadNoise(pt._ctx, -1, tiles.ctypes.data, tiles.nbytes, C.addressof(s)) == INVALID_OPERATION
    pt.Dispose()
    # a context that holds a shard of the rows, and a multi-device context
    from idkengine_amd.pathtracer import PathTracer
    shard = PathTracer(w, h, row_modulo=2, row_remainder=0)
    assert shard._L.idkptSetNoiseEstimate(shard._ctx, 1) == INVALID_OPERATION and shard._L.idkptSetNoiseEstimate(shard._ctx, 0) == 0 and not shard.GetNoiseEstimate()
    shard.Dispose()
    group = PathTracer(w, h, devices=[0, 0])
    assert group._L.idkptSetNoiseEstimate(group._ctx, 1) == INVALID_OPERATION and group._L.idkptSetNoiseEstimate(group._ctx, 0) == 0 and not group.GetNoiseEstimate()
    assert c_estimate(group) == INVALID_OPERATION
    group.Dispose()
