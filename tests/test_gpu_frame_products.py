"""The life cycle the four frame products share — the display image (idkptPresent), the bloom chains and expanded image (idkptBloom), the denoised image
(idkptDenoise) and the noise estimate with its moments images (idkptEstimateNoise) — across all four at once, in ONE context: buffers that belong to a ring slot and a
frame size, are made at first use, end in 64 guard bytes of 0xA5, are kept by idkptSetMaxBatch, released by every resize (display and bloom by
idkptSetPresentationSize too), and live on one device that holds the whole frame.  What each product computes is held to its restatement by the product's own file
(test_gpu_present.py, test_gpu_present_scaled.py, test_gpu_bloom.py, test_gpu_denoise.py, test_gpu_noise.py); here only bits before against bits after, guards, sizes and
refusals are looked at.

21 x 13 is no multiple of 4 or 8: idkptPresent has a row tail and the noise estimate has tiles cut at both edges.  Ring of 2, OutputAOVs 1, the noise estimate on, the
32-triangle Cornell box of test_gpu_noise.py, 2 and 3 samples in the two slots."""
import ctypes as C
import os
import sys
import numpy as np

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_present import c_present  # noqa: E402
from test_gpu_present_scaled import device_display, expanded, chain_with_guard, get_pres  # noqa: E402
from test_gpu_bloom import c_bloom, c_info, c_level  # noqa: E402
from test_gpu_denoise import c_denoise, denoised_and_guard  # noqa: E402
from test_gpu_noise import new_pt, moments_and_guard, noise_and_guards, c_estimate  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
OK, INVALID_OPERATION = 0, 3
RGBA8, RGBA32F = T.IDKPT_DISPLAY_RGBA8, T.IDKPT_DISPLAY_RGBA32F
W, H = 21, 13


def render(pt, ring):
    """slot q accumulates 2 + q samples"""
    for q in range(ring):
        assert pt.BeginFrame() == q
        for _ in range(2 + q):
            pt.Compute()


def make_all(pt, ring):
    """every product of every slot (the denoised image first: the result source may ask for it)"""
    for q in range(ring):
        pt._check(c_denoise(pt, T.Denoise(Iterations=3), q))          # three iterations: both images the iterations alternate between are used
        pt._check(c_estimate(pt, slot=q))
        pt._check(c_present(pt, T.TonemapSettings(), RGBA32F, slot=q))
        pt._check(c_present(pt, T.TonemapSettings(), RGBA8, slot=q))   # (the guard moves to the end of the smaller image; the allocation stays)
        pt._check(c_bloom(pt, T.BloomSettings(), slot=q))


def products(pt, ring, pw, ph):
    """the bits of every product of every slot, read through the device pointers with their 64 guard bytes (asserted 0xA5) — display, bloom expanded, both bloom
    chains, denoised, tile map, summary, moments — and the accumulated images"""
    out = []
    for q in range(ring):
        disp, guard = device_display(pt, RGBA8, pw, ph, q)
        assert (guard == 0xA5).all(), q
        exp, guard, _ = expanded(pt, pw, ph, q)
        assert (guard == 0xA5).all(), q
        chains = []
        for chain in (0, 1):
            body, guard = chain_with_guard(pt, chain, q)
            assert (guard == 0xA5).all(), (q, chain)
            chains.append(body)
        levels, w0, h0 = c_info(pt, q)
        assert (w0, h0) == (pw // 2, ph // 2) and levels >= 2
        level = [c_level(pt, chain, l, q) for chain in (0, 1) for l in range(levels - chain)]   # (the downloads agree with the chains as they lie in memory)
        assert b"".join(x.tobytes() for x in level[:levels]) == chains[0].tobytes() and b"".join(x.tobytes() for x in level[levels:]) == chains[1].tobytes()
        den, guard = denoised_and_guard(pt, q)
        assert (guard == 0xA5).all(), q
        tiles, summary = noise_and_guards(pt, q)                        # (asserts both guards itself)
        assert tiles.shape == ((pt.height + 7) // 8, (pt.width + 7) // 8, 2) and summary["Samples"] == 2 + q
        mom, guard = moments_and_guard(pt, q)
        assert (guard == 0xA5).all(), q
        out.append(dict(display=disp, expanded=exp, down=chains[0], up=chains[1], denoised=den, tiles=tiles, summary=np.array([summary["TilesAbove"], summary["Tiles"], summary["Samples"], int(np.float32(summary["MaxTileMean"]).view(np.uint32))], np.uint64),
                        moments=mom, images=np.stack([pt.FrameResult(q, i) for i in range(3)])))
    return out


def unchanged(a, b, keys=None):
    assert len(a) == len(b)
    for q, (x, y) in enumerate(zip(a, b)):
        for k in (keys or x.keys()):
            assert x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), (q, k)


def refusals(pt, ring):
    """(display, bloom, denoised, noise) per slot, the current one (-1) last: True where EVERY call that reads the product answers IDKPT_ERR_INVALID_OPERATION ("the slot holds
    none since the last resize"), False where none does (the downloads are given a wrong size on purpose: a slot that holds the product answers INVALID_ARGUMENT, after the look-up)"""
    out = []
    p = C.c_void_p(); n = C.c_size_t(); lv = C.c_int32(); r = C.c_int32(); buf = np.zeros(8, np.uint8)
    L, c = pt._L, pt._ctx
    for q in list(range(ring)) + [-1]:
        rcs = ([L.idkptGetDisplayDevicePtr(c, q, C.byref(p), C.byref(n)), L.idkptDownloadDisplay(c, q, buf.ctypes.data, buf.nbytes)],
               [L.idkptGetBloomDevicePtr(c, q, C.byref(p), C.byref(n)), L.idkptGetBloomChainDevicePtr(c, q, 0, C.byref(p), C.byref(n)), L.idkptGetBloomInfo(c, q, C.byref(lv), None, None),
                L.idkptGetBloomRoute(c, q, C.byref(r)), L.idkptDownloadBloom(c, q, 0, 0, buf.ctypes.data, buf.nbytes)],
               [L.idkptGetDenoisedDevicePtr(c, q, C.byref(p), C.byref(n)), L.idkptDownloadDenoised(c, q, buf.ctypes.data, buf.nbytes), L.idkptGetDenoiseRoute(c, q, 0, C.byref(r))],
               [L.idkptGetNoiseDevicePtr(c, q, C.byref(p), None, C.byref(n)), L.idkptDownloadNoise(c, q, buf.ctypes.data, buf.nbytes, None)])
        for one in rcs:
            assert all(rc == INVALID_OPERATION for rc in one) or INVALID_OPERATION not in one, (q, rcs)
        out.append(tuple(one[0] == INVALID_OPERATION for one in rcs))
    return out


def test_the_four_products_share_one_life_cycle(native_builder):
    sc = S.cornell_scene(native_builder, variant="diffuse", sky_color=(0.4, 0.6, 0.9))
    pt = new_pt(sc, W, H, noise=True, aovs=1, max_batch=2, ring=2)
    assert refusals(pt, 2) == [(True,) * 4] * 3                        # nothing is made before its first use
    render(pt, 2)
    make_all(pt, 2)
    before = products(pt, 2, W, H)
    assert before[0]["display"].shape == (H, W, 4) and before[0]["images"].any() and before[1]["moments"].any()
    pt.SetResultSource(T.IDKPT_RESULT_DENOISED)

    # idkptSetMaxBatch: the wavefront buffers are re-made; every product of both slots and the accumulated images keep their bits
    pt.set_max_batch(3)
    unchanged(products(pt, 2, W, H), before)
    assert pt.GetNoiseEstimate() and pt.GetResultSource() == T.IDKPT_RESULT_DENOISED

    # idkptSetPresentationSize: what has the presentation size goes (display, bloom); the rest keeps its bits
    pt.SetPresentationSize(10, 7)
    assert refusals(pt, 2) == [(True, True, False, False)] * 3
    for q in range(2):
        pt._check(c_present(pt, T.TonemapSettings(), RGBA32F, slot=q)); pt._check(c_present(pt, T.TonemapSettings(), RGBA8, slot=q))
        pt._check(c_bloom(pt, T.BloomSettings(), slot=q))
    after = products(pt, 2, 10, 7)                                     # (sizes of 10 x 7 and intact guards are asserted there)
    unchanged(after, before, ("denoised", "tiles", "summary", "moments", "images"))
    assert after[0]["display"].shape == (7, 10, 4) and after[0]["expanded"].shape == (7, 10, 4)

    # idkptSetFrameRing, then idkptSetSize: everything goes; the switches stay; the moments images are zeroed at their first use
    for ring, resize in ((3, lambda: pt.SetFrameRing(3)), (3, lambda: pt.SetSize(13, 9))):
        state = (get_pres(pt), pt.GetResultSource(), pt.GetNoiseEstimate())
        assert state == ((10, 7), T.IDKPT_RESULT_DENOISED, True)
        resize()
        assert refusals(pt, ring) == [(True,) * 4] * (ring + 1)
        assert (get_pres(pt), pt.GetResultSource(), pt.GetNoiseEstimate()) == state
        for q in range(ring):
            mom, guard = moments_and_guard(pt, q)
            assert mom.shape == (pt.height, pt.width, 4) and not mom.any() and (guard == 0xA5).all(), q
        render(pt, ring)
        make_all(pt, ring)
        products(pt, ring, 10, 7)

    # a row-layout call that leaves a shard switches the noise estimate off; the denoised image needs the whole frame
    pt.SetRowRange(2, 5)
    assert not pt.GetNoiseEstimate()
    assert c_denoise(pt, T.Denoise(Iterations=3), 0) == INVALID_OPERATION
    assert refusals(pt, 3) == [(True,) * 4] * 4
    pt.SetRowRange(0, 9)                                               # the whole frame again: everything can be made
    assert not pt.GetNoiseEstimate()
    pt.SetNoiseEstimate(True)
    render(pt, 3)
    make_all(pt, 3)
    products(pt, 3, 10, 7)

    assert pt._L.idkptDestroy(pt._ctx) == OK
    pt._ctx = None
