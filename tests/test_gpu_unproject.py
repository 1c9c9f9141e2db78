"""idkptUnprojectSky on the device (csrc/kernels_unproject.hpp, csrc/unproject_texel.hpp): an equirectangular panorama becomes the sky's resident faces as
SkyBoxManager.LoadSkyBoxEquirectangular makes them.  The device is held to the bound tests/test_unproject_ref.py measures per case (2 x the larger error of the two binary32
executions of the reference material against the binary64 evaluation, scaled per texel; a stored half must lie in rtz(T -+ b scale)), with T evaluated from the
library's own packed texels (round to nearest even: the fixture's texels bit for bit in every three-channel case).  Frames, ordering, refusals and the 2-member context
follow tests/test_gpu_sky.py."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import unproject_ref as R  # noqa: E402
from test_unproject_ref import case_bound, within_any  # noqa: E402
from test_gpu_sky import CAM, W, H, new_pt, frame, fresh_frame, with_sky, same, random_faces  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3


@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, variant="diffuse", sky_color=(0.2, 0.3, 0.5))


@pytest.fixture(scope="module")
def bounds():
    fx = R.load_fixture()
    return [case_bound(fx, c)[0] for c in range(len(R.CASES))]


@pytest.fixture(scope="module")
def pt(scene):
    p = new_pt(scene)
    yield p
    p.Dispose()


def srgb_store(rgba):
    """SrgbToLinear in binary32 on a packed texel's R, G, B and the half store, expanded: the resident texel where all four taps are that texel"""
    v = np.asarray(rgba, np.float32).copy()
    v[..., :3] = R.srgb_to_linear(v[..., :3], np.float32)
    return R.half_values(R.rtz_half(v), np.float32)


def alpha_is_one(faces):
    """alpha 1.0 through the filter: (1 - a) + a is 1 or one binary32 ulp below it, which the store truncates to the half below 1 (llvmpipe forms the sum otherwise and holds 1.0 everywhere; SampleSky reads R, G, B only)"""
    return bool(((faces[..., 3] == 1.0) | (faces[..., 3] == np.float32(1.0 - 2.0 ** -11))).all())


def test_every_case_within_the_measured_bound(pt, bounds):
    for c, case in enumerate(R.CASES):
        Wp, Hp, S_, ch, arg = case
        img = R.input_image(case)
        pt.UnprojectSky(img, arg if arg else None)
        got = pt.DownloadSky()
        assert got.shape == (6, S_, S_, 4) and got.dtype == np.float32          # skySize as specified
        assert R.is_half(got).all(), c                                          # every resident value is exactly a half
        packed = R.pack(img)
        ev = R.evaluate64(packed, S_)
        m = R.seam_mask(S_)
        got_bits = got.astype(np.float16).view(np.uint16)
        np32 = R.half_values(R.rtz_half(R.unproject(packed, S_, np.float32)[0]), np.float32)
        steps = np.abs(got_bits.astype(np.int64) - np32.astype(np.float16).view(np.uint16).astype(np.int64)).max()
        print(f"case {c + 1} {case}: b = {bounds[c]:.3e}  texels equal to the restatement bit for bit: {float((got == np32).all(axis=-1).mean()):.3f}  largest distance: {int(steps)} half step(s)")
        ok = within_any(got_bits, ev, bounds[c], S_)
        assert ok.all(), (c, int((~ok).sum()))
        if m.any():                                                             # C's signed zeros: the first evaluation alone holds at the seam texels
            assert R.halves_within(got_bits, ev[0][0], ev[0][1], bounds[c])[m].all(), c
        if ch == 3:
            assert alpha_is_one(got)


def test_trivial_filters_give_exact_texels(pt):
    # a constant image: every tap is the same half x, and mix(mix(x, x, ax), mix(x, x, ax), ay) is x within two binary32 ulps whatever the weights are (x a power of two:
    # both products are exact, (1 - a) + a rounds twice).  The constants are chosen so that every binary32 value that close to x has the same stored half — checked
    # here —, so the expected texel is exact: SrgbToLinear (both branches) of the packed half, truncated.
    const = np.array([0.5, 0.03125, 2.0], np.float32)
    want = srgb_store(np.append(const, 1.0))
    for k in (-2, -1, 1, 2):
        near = (const.astype(np.float64) * (1 + k * 2.0 ** -23)).astype(np.float32)
        assert same(srgb_store(np.append(near, 1.0))[:3], want[:3])
    img = np.broadcast_to(const, (8, 16, 3)).copy()
    pt.UnprojectSky(img, 4)
    got = pt.DownloadSky()
    assert got.shape == (6, 4, 4, 4) and (got[..., :3] == want[:3]).all() and alpha_is_one(got)
    # zeros stay zeros, whatever the weights
    pt.UnprojectSky(np.zeros((8, 16, 3), np.float32), 4)
    z = pt.DownloadSky()
    assert (z[..., :3] == 0.0).all() and alpha_is_one(z)
    # one-hot: one texel in a black image — the packed value, the tap indices and the weights together.  A cube texel that has it among its taps holds
    # store(SrgbToLinear(v * wx * wy)), every other texel exactly 0.  The weights come from atan2f / asinf and the upper branch from powf, whose last bits differ
    # between correct libraries; the hot texel and its three values (both branches of SrgbToLinear occur) are chosen so that the stored halves do not depend on them:
    # checked here by moving u and v up to 4 units in the last place each way (an atan2f or asinf 4 ulp off moves u or v by less: * 0.1591 / 0.3183, + 0.5) and the value
    # in front of the store by 4 more.  The expected halves are therefore exact, and the device must show them bit for bit.
    hot = np.zeros((8, 16, 3), np.float32); hot[3, 5] = (1.0, 0.75, 3.0)
    packed = R.pack(hot)
    value = R.unproject(packed, 4, np.float32)[0][..., :3]
    want = R.rtz_half(value)
    for du in range(-4, 5):
        for dv in range(-4, 5):
            near = R.unproject(packed, 4, np.float32, uv_ulps=(du, dv))[0][..., :3]
            for k in (-4, 0, 4):
                assert (R.rtz_half(np.where(near != 0, R.shift_ulps(near, k), near)) == want).all(), (du, dv, k)
    touched = (want != 0).all(axis=-1)
    assert 3 <= int(touched.sum()) < touched.size and (want[~touched] == 0).all()
    assert ((value[touched] < 0.0031) & (value[touched] > 0)).any() and (value[touched] > 0.0032).any()      # c / 12.92 and the power, both
    pt.UnprojectSky(hot, 4)
    got = pt.DownloadSky()
    assert same(got[..., :3].astype(np.float16).view(np.uint16), want) and R.is_half(got).all() and alpha_is_one(got)
    # ... and exactly the packed half where the weights are trivial: S = 1 looks along each axis; +X has u = v = 0.5, whose four taps of a 2 x 2 panorama are its four
    # texels with weights 0.5 exactly (f = 0.5): the mean of the halves, in binary32
    quad = np.array([[[1.0, 0.25, 3.0], [0.5, 0.75, 1.0]], [[2.0, 0.125, 5.0], [0.5, 0.875, 7.0]]], np.float32)
    pt.UnprojectSky(quad, 1)
    got = pt.DownloadSky()
    mean = (quad[0, 0] * np.float32(0.5) + quad[0, 1] * np.float32(0.5)) * np.float32(0.5) + (quad[1, 0] * np.float32(0.5) + quad[1, 1] * np.float32(0.5)) * np.float32(0.5)
    assert got.shape == (6, 1, 1, 4) and same(got[0, 0, 0], srgb_store(np.append(mean, 1.0)))


def test_face_size_zero_is_width_over_four(pt):
    img = R.input_image(R.CASES[3])                                             # 24 x 16
    pt.UnprojectSky(img, None); a = pt.DownloadSky()
    pt.UnprojectSky(img, 6); b = pt.DownloadSky()
    pt.UnprojectSky(np.ascontiguousarray(img[:, :23]), 0); c = pt.DownloadSky()   # 23 // 4 = 5
    assert a.shape == (6, 6, 6, 4) and same(a, b) and c.shape == (6, 5, 5, 4)


def test_beyond_65504_saturates(pt):
    """the library's rule, not the reference's: a finite input beyond the half range is stored as +-65504; so is a result beyond it"""
    img = np.zeros((4, 8, 3), np.float32)
    img[..., 0] = 1e6; img[..., 1] = 65520.0; img[..., 2] = 3.0e38
    pt.UnprojectSky(img, 2)
    got = pt.DownloadSky()
    assert np.isfinite(got).all() and (got[..., :3] == 65504.0).all() and alpha_is_one(got)
    img4 = np.zeros((4, 8, 4), np.float32); img4[..., 3] = -1e9; img4[..., 0] = 65519.0
    pt.UnprojectSky(img4, 2)
    got = pt.DownloadSky()
    assert np.isfinite(got).all() and ((got[..., 3] == -65504.0) | (got[..., 3] == -65472.0)).all() and (got[..., 0] == 65504.0).all()   # (alpha is filtered, not transformed: -65504 or, where (1 - a) + a fell one ulp short, the half below)


def test_three_channels_equal_four_with_alpha_one(pt):
    img = R.input_image(R.CASES[2])                                             # 18 x 9: texels % 4 != 0, the scalar tail of the three-channel pack
    img4 = np.concatenate([img, np.ones(img.shape[:2] + (1,), np.float32)], axis=2)
    pt.UnprojectSky(img); a = pt.DownloadSky()
    pt.UnprojectSky(img4); b = pt.DownloadSky()
    assert same(a, b)
    odd = R.input_image(R.CASES[1])[:7, :19]                                    # 133 texels: one texel in the tail
    odd = np.ascontiguousarray(odd)
    pt.UnprojectSky(odd, 3); a = pt.DownloadSky()
    pt.UnprojectSky(np.concatenate([odd, np.ones(odd.shape[:2] + (1,), np.float32)], axis=2), 3); b = pt.DownloadSky()
    assert same(a, b)


def test_frame_after_the_call_is_the_frame_of_the_downloaded_faces(scene, pt):
    img = R.input_image(R.CASES[1])
    img = np.minimum(np.abs(img), 8.0)                                          # (a picture, not a stress test: radiance of a few units)
    pt.UnprojectSky(img)
    faces = pt.DownloadSky()
    a = frame(pt)
    pt.UpdateSky(None); pt.UpdateSky(faces)
    b = frame(pt)
    assert faces.shape == (6, 5, 5, 4) and same(a, b) and same(a, fresh_frame(scene, faces))
    assert a[..., :3].max() > 0


@pytest.mark.parametrize("defer_last", (0, 1))
def test_call_is_ordered_behind_queued_samples(scene, defer_last):
    old = random_faces(4, 1)
    img = np.minimum(np.abs(R.input_image(R.CASES[0])), 8.0)
    p = new_pt(with_sky(scene, old), defer_last=defer_last)
    p.set_max_batch(4); p.SetFrameRing(2)
    a = p.BeginFrame(); p.Compute(); p.Compute()                                # two samples queued under the old sky ...
    assert p._L.idkptUnprojectSky(p._ctx, 16, 8, 3, img.ctypes.data, 0) == 0    # ... no flush by the host
    b = p.BeginFrame(); p.ResetAccumulation(); p.Compute(); p.Compute()
    first, last = p.FrameResult(a), p.FrameResult(b)
    new = p.DownloadSky()
    p.Dispose()
    assert same(first, fresh_frame(scene, old, samples=2, defer_last=defer_last))
    assert same(last, fresh_frame(scene, new, samples=2, defer_last=defer_last))
    assert not same(first, last)


def test_refusals_leave_the_old_sky_resident(scene, pt):
    from idkengine_amd.pathtracer import PathTracer
    img = R.input_image(R.CASES[0])
    empty = PathTracer(W, H)
    assert empty._L.idkptUnprojectSky(empty._ctx, 16, 8, 3, img.ctypes.data, 0) == INVALID_OPERATION
    empty.Dispose()
    pt.UpdateSky(random_faces(3, 21))
    faces, before = pt.DownloadSky(), frame(pt)
    L, ctx = pt._L, pt._ctx
    nan = img.copy(); nan[7, 15, 2] = np.nan
    inf = img.copy(); inf[0, 0, 0] = -np.inf
    three = np.ascontiguousarray(img[:, :3])
    two = np.zeros((8, 16, 2), np.float32)
    failing = [("width 3 with faceSize 0", lambda: L.idkptUnprojectSky(ctx, 3, 8, 3, three.ctypes.data, 0)), ("channels 2", lambda: L.idkptUnprojectSky(ctx, 16, 8, 2, two.ctypes.data, 0)),
               ("NaN texel", lambda: L.idkptUnprojectSky(ctx, 16, 8, 3, nan.ctypes.data, 0)), ("infinite texel", lambda: L.idkptUnprojectSky(ctx, 16, 8, 3, inf.ctypes.data, 0)),
               ("faceSize 4097", lambda: L.idkptUnprojectSky(ctx, 16, 8, 3, img.ctypes.data, 4097)), ("faceSize -1", lambda: L.idkptUnprojectSky(ctx, 16, 8, 3, img.ctypes.data, -1)),
               ("width 0", lambda: L.idkptUnprojectSky(ctx, 0, 8, 3, img.ctypes.data, 4)), ("width 16385", lambda: L.idkptUnprojectSky(ctx, 16385, 8, 3, img.ctypes.data, 4)),
               ("height 8193", lambda: L.idkptUnprojectSky(ctx, 16, 8193, 3, img.ctypes.data, 4)), ("null pixels", lambda: L.idkptUnprojectSky(ctx, 16, 8, 3, None, 0))]
    for name, call in failing:
        assert call() == INVALID_ARGUMENT, name
        msg = C.c_char_p(); L.idkptGetLastError(ctx, C.byref(msg))
        assert (msg.value or b"").decode().startswith("idkptUnprojectSky:"), (name, msg.value)
        assert same(pt.DownloadSky(), faces) and same(frame(pt), before), name
    assert L.idkptUnprojectSky(ctx, 3, 8, 3, three.ctypes.data, 2) == 0         # width 3 is fine with an explicit size
    assert pt.DownloadSky().shape == (6, 2, 2, 4)
    with pytest.raises(TypeError):
        pt.UnprojectSky(img.astype(np.float64))
    with pytest.raises(ValueError):
        pt.UnprojectSky(np.zeros((8, 16, 2), np.float32))
    with pytest.raises(ValueError):
        pt.UnprojectSky(np.zeros((8, 16, 6), np.float32)[..., ::2])


def test_two_members_on_one_gpu(scene, pt):
    img = np.minimum(np.abs(R.input_image(R.CASES[4])), 8.0)
    two = new_pt(scene, devices=[0, 0])
    pt.UnprojectSky(img, 9); two.UnprojectSky(img, 9)
    a, b = frame(pt), frame(two)                                                # rows alternate between the members: both skies are sampled
    assert same(pt.DownloadSky(), two.DownloadSky()) and same(a, b)
    two.UpdateSky(None); two.UnprojectSky(np.ascontiguousarray(img[:, :20]))    # again, smaller, after no sky
    pt.UnprojectSky(np.ascontiguousarray(img[:, :20]))
    assert same(pt.DownloadSky(), two.DownloadSky()) and same(frame(pt), frame(two))
    two.Dispose()
