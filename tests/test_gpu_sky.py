"""The sky without a scene upload: idkptComputeSky (the procedural atmosphere on the device, csrc/kernels_sky.hpp), idkptUpdateSky (host faces, float or 8-bit) and
idkptDownloadSky.  The atmosphere is held to the bound tests/test_sky_ref.py measures (2 x the larger error of the two binary32 executions of the reference material, per
case, computed from the fixture at run time); everything else — which sky a frame is rendered with, the order against queued samples, the 8-bit expansion, failures, a
two-member context — is bit for bit."""
import copy
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import sky_ref as R  # noqa: E402
from test_sky_ref import sky_bound  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import bits  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 64, 48
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def atmosphere_of(case):
    return T.Atmosphere(*case[1:])


def with_sky(sc, faces):
    out = copy.copy(sc)
    out.sky_faces = None if faces is None or faces.shape[1] == 0 else np.ascontiguousarray(faces, np.float32)
    return out


def six_colours():
    sky = np.zeros((6, 1, 1, 4), np.float32)
    sky[:, 0, 0, :3] = [(0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.2, 0.3, 0.9), (0.7, 0.7, 0.1), (0.1, 0.6, 0.7), (0.8, 0.1, 0.8)]
    sky[..., 3] = 1.0
    return sky


def random_faces(S_, seed):
    rng = np.random.default_rng(seed)
    f = np.ones((6, S_, S_, 4), np.float32); f[..., :3] = rng.uniform(0.0, 2.0, (6, S_, S_, 3)).astype(np.float32)
    return f


@pytest.fixture(scope="module")
def scene(native_builder):
    """The Cornell box seen from far enough that the 64 x 48 frame holds 8 x 8 tiles of sky only, of surfaces only and of both; the open front lets the sky light it."""
    return S.cornell_scene(native_builder, variant="diffuse", sky_color=(0.2, 0.3, 0.5))


CAM = S.Camera(W, H, position=(0.6, 0.4, 7.0), view_dir=(-0.08, -0.05, -1.0), fovy_deg=40.0)


def new_pt(sc, depth=3, devices=None, **options):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(W, H, devices=devices)
    for k, v in options.items():
        pt.set_option(k, v)
    if sc is not None:
        pt.UploadScene(sc)
    pt.SetCamera(CAM); pt.RayDepth = depth
    return pt


def frame(pt, samples=1):
    pt.ResetAccumulation()
    for _ in range(samples):
        pt.Compute()
    return pt.Result


def fresh_frame(sc, faces, samples=1, **options):
    pt = new_pt(with_sky(sc, faces), **options)
    img = frame(pt, samples)
    pt.Dispose()
    return img


@pytest.fixture(scope="module")
def reference():
    """[(case, fixture, binary32 restatement, binary64 evaluation)] — computed once for the module."""
    return [(case, fx, R.atmosphere(*case, dtype=np.float32), R.atmosphere(*case, dtype=np.float64)) for case, fx in R.load_fixture()]


def test_compute_sky_within_the_measured_bound(scene, reference):
    pt = new_pt(scene)
    for k, (case, fx, f32, f64) in enumerate(reference):
        pt.ComputeSky(case[0], atmosphere_of(case))
        got = pt.DownloadSky()
        bound, e_gl, e_np = sky_bound(fx, f32, f64)
        e_dev = R.err(got, f64)
        print(f"case {k + 1} {case}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {bound:.3e}  e_device = {e_dev:.3e}  texels equal to the fixture bit for bit: {float((bits(got) == bits(fx)).all(axis=-1).mean()):.3f}")
        assert got.shape == fx.shape and got.dtype == np.float32 and np.isfinite(got).all()
        assert (got[..., 3] == 1.0).all()
        assert e_dev <= bound, (k, e_dev, bound)
        if case[3] == 0.0:
            assert (got[..., :3] == 0.0).all()
    pt.Dispose()


def test_installed_sky_is_the_sky(scene, oracle_mod):
    pt = new_pt(scene)
    pt.ComputeSky(8, atmosphere_of(R.LOW_SUN))
    img = frame(pt)
    faces = pt.DownloadSky()
    n_primary = pt.stats()["alive_counts"][0]
    assert faces.shape == (6, 8, 8, 4) and faces[..., :3].max() > 0.1
    assert 0 < n_primary < W * H                                        # some pixels never reach the traversal (sky tiles, class 8), the others do: test_view_has_sky_surface_and_mixed_tiles
    # a fresh context that gets the same faces through idkptUploadScene, and the oracle given those faces
    assert same(img, fresh_frame(scene, faces))
    o = oracle_mod.OraclePathTracer(with_sky(scene, faces), W, H); o.set_camera(CAM); o.settings.RayDepth = 3; o.render()
    assert same(img, o.image(0))
    o.close()
    # the same through idkptUpdateSky(float faces), after another sky was resident
    pt.UpdateSky(six_colours())
    assert not same(frame(pt), img)
    pt.UpdateSky(faces)
    assert same(pt.DownloadSky(), faces) and same(frame(pt), img)
    pt.Dispose()


def test_view_has_sky_surface_and_mixed_tiles(scene):
    """The premise of the frame tests: primary hits per 8 x 8 tile are 0 somewhere, 64 somewhere and in between somewhere."""
    pt = new_pt(scene, depth=1); pt.enable_primary_hit_capture(True); pt.Compute()
    _, tri, _ = pt.primary_hits()
    hit = (tri.reshape(H, W) != 0xFFFFFFFF).reshape(H // 8, 8, W // 8, 8).sum(axis=(1, 3))
    pt.Dispose()
    assert (hit == 0).any() and (hit == 64).any() and ((hit > 0) & (hit < 64)).any()


@pytest.mark.parametrize("no_tile_cull", (0, 1))
def test_class_transitions_in_one_context(scene, no_tile_cull):
    """S = 1 (tile classes 1-6) -> textured (8) -> S = 1 -> none (7) -> textured, odd size: every frame is the frame of a context that never held another sky."""
    pt = new_pt(with_sky(scene, six_colours()), no_tile_cull=no_tile_cull)
    other = six_colours()[::-1].copy()
    steps = [("uploaded S = 1", lambda: None), ("ComputeSky(16)", lambda: pt.ComputeSky(16, T.Atmosphere(12, 4, 15.0, 0.3, 1.2))), ("UpdateSky(S = 1)", lambda: pt.UpdateSky(other)),
             ("UpdateSky(None)", lambda: pt.UpdateSky(None)), ("ComputeSky(5)", lambda: pt.ComputeSky(5, atmosphere_of(R.LOW_SUN)))]
    seen = []
    for name, step in steps:
        step()
        img = frame(pt)
        faces = pt.DownloadSky()
        assert same(img, fresh_frame(scene, faces, no_tile_cull=no_tile_cull)), name
        seen.append((faces.shape[1], img))
    assert [s for s, _ in seen] == [1, 16, 1, 0, 5]
    assert not same(seen[0][1], seen[2][1]) and not same(seen[1][1], seen[4][1]) and not same(seen[3][1], seen[0][1])
    pt.Dispose()


@pytest.mark.parametrize("defer_last", (0, 1))
def test_update_is_ordered_behind_queued_samples(scene, defer_last):
    old, new = random_faces(4, 1), random_faces(3, 2)
    pt = new_pt(with_sky(scene, old), defer_last=defer_last)
    pt.set_max_batch(4); pt.SetFrameRing(2)
    a = pt.BeginFrame(); pt.Compute(); pt.Compute()                      # two samples queued under the old sky ...
    pt.UpdateSky(new)                                                    # ... no flush by the host
    b = pt.BeginFrame(); pt.ResetAccumulation(); pt.Compute(); pt.Compute()   # (the accumulation is the host's to reset; the ring keeps the first two samples' image readable)
    first, last = pt.FrameResult(a), pt.FrameResult(b)
    pt.Dispose()
    assert same(first, fresh_frame(scene, old, samples=2, defer_last=defer_last))
    assert same(last, fresh_frame(scene, new, samples=2, defer_last=defer_last))
    assert not same(first, last)


def test_ray_state_of_the_sample_before_the_update_survives(scene):
    """defer_last (the default) and the tile classes leave radiance that is only produced on demand — from the sky: it must be produced from the OLD one."""
    old, new = random_faces(4, 3), random_faces(4, 4)
    twin = new_pt(with_sky(scene, old)); twin.Compute()
    want_rays, want_queue = twin.rays(), twin.alive_queue()
    twin.Dispose()
    for update in (lambda p: p.UpdateSky(new), lambda p: p.ComputeSky(4, T.Atmosphere()), lambda p: p.UpdateSky(None)):
        pt = new_pt(with_sky(scene, old)); pt.Compute()
        update(pt)
        assert pt.rays().tobytes() == want_rays.tobytes() and (pt.alive_queue() == want_queue).all()
        pt.Dispose()


def test_8bit_faces(scene):
    rng = np.random.default_rng(7)
    raw = rng.integers(0, 256, (6, 4, 4, 4), dtype=np.uint8)
    pt = new_pt(scene)
    for fmt, expand in ((T.IDKPT_TEXFMT_SRGB8_A8, R.srgb8_to_float), (T.IDKPT_TEXFMT_RGBA8, R.unorm8_to_float)):
        want = expand(raw)
        pt.UpdateSky(raw, fmt)
        assert same(pt.DownloadSky(), want), fmt
        img = frame(pt)
        pt.UpdateSky(None); pt.UpdateSky(want)
        assert same(frame(pt), img), fmt
    assert not same(R.srgb8_to_float(raw), R.unorm8_to_float(raw))
    # the Python layer checks the array against the format: the library only sees a pointer
    with pytest.raises(TypeError):
        pt.UpdateSky(raw)                                                # uint8 as RGBA32F
    with pytest.raises(TypeError):
        pt.UpdateSky(raw.astype(np.float32), T.IDKPT_TEXFMT_RGBA8)
    with pytest.raises(ValueError):
        pt.UpdateSky(np.zeros((6, 4, 3, 4), np.float32))
    with pytest.raises(ValueError):
        pt.UpdateSky(np.zeros((6, 4, 4, 8), np.float32)[..., ::2])       # not contiguous
    with pytest.raises(ValueError):
        pt.UpdateSky(raw, 5)
    pt.Dispose()


def test_errors_leave_the_state_alone(scene):
    from idkengine_amd.pathtracer import PathTracer
    empty = PathTracer(W, H)                                             # no scene yet: all three refuse
    a = T.Atmosphere(); s = C.c_int32(-7); f = random_faces(2, 5)
    assert empty._L.idkptComputeSky(empty._ctx, 8, C.addressof(a)) == INVALID_OPERATION
    assert empty._L.idkptUpdateSky(empty._ctx, 2, T.IDKPT_TEXFMT_RGBA32F, f.ctypes.data) == INVALID_OPERATION
    assert empty._L.idkptDownloadSky(empty._ctx, C.byref(s), None, 0) == INVALID_OPERATION
    empty.Dispose()

    pt = new_pt(scene)
    pt.ComputeSky(4, atmosphere_of(R.LOW_SUN))
    faces, img = pt.DownloadSky(), frame(pt)
    L, ctx = pt._L, pt._ctx

    def atmo(**kw):
        x = T.Atmosphere()
        for k, v in kw.items():
            setattr(x, k, v)
        return x
    buf = np.zeros(faces.size, np.float32)
    failing = [
        ("idkptComputeSky", "faceSize 0", lambda: L.idkptComputeSky(ctx, 0, C.addressof(a))), ("idkptComputeSky", "faceSize -1", lambda: L.idkptComputeSky(ctx, -1, C.addressof(a))),
        ("idkptComputeSky", "faceSize 4097", lambda: L.idkptComputeSky(ctx, 4097, C.addressof(a))), ("idkptComputeSky", "ISteps 0", lambda: L.idkptComputeSky(ctx, 8, C.addressof(atmo(ISteps=0)))),
        ("idkptComputeSky", "JSteps 4097", lambda: L.idkptComputeSky(ctx, 8, C.addressof(atmo(JSteps=4097)))), ("idkptComputeSky", "NaN elevation", lambda: L.idkptComputeSky(ctx, 8, C.addressof(atmo(Elevation=float("nan"))))),
        ("idkptComputeSky", "infinite intensity", lambda: L.idkptComputeSky(ctx, 8, C.addressof(atmo(LightIntensity=float("inf"))))), (None, "null settings", lambda: L.idkptComputeSky(ctx, 8, None)),
        ("idkptUpdateSky", "format 5", lambda: L.idkptUpdateSky(ctx, 2, 5, f.ctypes.data)), ("idkptUpdateSky", "faceSize -1", lambda: L.idkptUpdateSky(ctx, -1, 0, f.ctypes.data)),
        ("idkptUpdateSky", "faceSize 4097", lambda: L.idkptUpdateSky(ctx, 4097, 0, f.ctypes.data)), ("idkptDownloadSky", "short destination", lambda: L.idkptDownloadSky(ctx, C.byref(s), buf.ctypes.data, buf.nbytes - 1)),
    ]
    for fn, name, call in failing:
        assert call() == INVALID_ARGUMENT, (fn, name)
        if fn is not None:
            msg = C.c_char_p(); L.idkptGetLastError(ctx, C.byref(msg))
            assert (msg.value or b"").decode().startswith(fn + ":"), (fn, name, msg.value)
        assert same(pt.DownloadSky(), faces) and same(frame(pt), img), (fn, name)
    assert L.idkptDownloadSky(ctx, C.byref(s), None, 0) == 0 and s.value == 4
    pt.Dispose()


def test_two_members_on_one_gpu(scene):
    raw = np.random.default_rng(9).integers(0, 256, (6, 3, 3, 4), dtype=np.uint8)
    one, two = new_pt(scene), new_pt(scene, devices=[0, 0])
    steps = [lambda p: p.ComputeSky(8, atmosphere_of(R.LOW_SUN)), lambda p: p.UpdateSky(random_faces(5, 11)), lambda p: p.UpdateSky(raw, T.IDKPT_TEXFMT_SRGB8_A8),
             lambda p: p.UpdateSky(None), lambda p: p.ComputeSky(3, T.Atmosphere(8, 2, 15.0, 1.0, 1.3))]
    frames = []
    for step in steps:
        step(one); step(two)
        a, b = frame(one), frame(two)
        assert same(one.DownloadSky(), two.DownloadSky()) and same(a, b)
        frames.append(a)
    assert not same(frames[0], frames[1]) and not same(frames[2], frames[3])
    one.Dispose(); two.Dispose()
