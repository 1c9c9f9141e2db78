"""The code that runs after a hit against the CPU oracle on ADVERSARIAL surfaces (tests/adversarial_surfaces.py; tests/test_adversarial_surfaces_ref.py proves on the CPU that the
classes take the branches they claim): ShadeHit behind k_shade_first, k_shade, k_shade_last + k_restore_last and the shading half of k_trace_fused, k_final_draw, and the surface
loop of k_shadows.  Every comparison is on bytes (gpu_helpers.assert_equal: image, AOVs, ray records, alive queue, primary hits, rays traced); the one exception is class
non_finite, compared with adversarial_surfaces.same_value.  Every variant of a (scene, settings) pair is held to one stored oracle answer, so the variants also equal each other.
A failure names the first differing pixel, the swatch class of its primary hit and the first differing field."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import adversarial_surfaces as A  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402,F401
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import assert_equal, bits  # noqa: E402

pytestmark = pytest.mark.gpu
_ORACLE = {}          # (case, frame, settings) -> the oracle's renderer, kept for the module: one answer per (scene, settings)


@pytest.fixture(scope="module", autouse=True)
def _close_the_oracles():
    yield
    for o in _ORACLE.values():
        o.close()
    _ORACLE.clear()


def _oracle(oracle_mod, key, sc, pf, w, h, overrides, frames, sequence=None):
    if key not in _ORACLE:
        o, _ = A.render_oracle(oracle_mod, sc, pf, w, h, overrides, frames, sequence=sequence)
        _ORACLE[key] = o
    return _ORACLE[key]


def _gpu(sc, pf, w, h, options, overrides, frames, batch, sequence=None):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h, settings=A.apply(T.Settings.default(), overrides))
    for k, v in options.items():
        pt.set_option(k, v)
    pt.UploadScene(sc); pt.SetPerFrameData(pf)
    pt.enable_counters(False); pt.enable_primary_hit_capture(True)
    if batch:
        pt.set_max_batch(batch)
    if sequence is not None:
        pt.SetSampleSequence(sequence, 1)
    for _ in range(frames):
        pt.Compute()
    pt.flush()
    return pt


def _hold(pt, o, sc, w, label):
    try:
        assert_equal(pt, o, aov=True, counters=False)
    except AssertionError:
        raise AssertionError(f"{label}: {A.first_difference(A.snapshot(pt), A.snapshot(o), sc, w)}") from None


CASES = [(c, f) for c in A.cases() for f in A.FRAMES]


@pytest.mark.parametrize("case,frame", CASES, ids=[f"{c[0]}-{f[0]}x{f[1]}" for c, f in CASES])
def test_frames_equal_the_oracle_under_every_variant(native_builder, oracle_mod, case, frame):
    """default, defer_last 0 / 1, the fused kernel, ray sorting, AOVs, three samples as one batch and one at a time, bounce_pixel_major 0 / 2, three accumulated frames and
    RayDepth 1, 2, 7, 20 — each alone from the case's own settings — on every form of the swatch room"""
    cid, _, form, use_tlas, cam, base = case
    w, h = frame
    sc = A.cached_room(form, native_builder); pf = A.case_camera(sc, cam, w, h)
    for label, options, ov, frames, batch in A.VARIANTS:
        d = dict(base, UseTlas=use_tlas); d.update(ov)
        o = _oracle(oracle_mod, (cid, frame, A.settings_key(d, {}, frames)), sc, pf, w, h, d, frames)
        pt = _gpu(sc, pf, w, h, options, d, frames, batch)
        try:
            _hold(pt, o, sc, w, f"{cid} {w}x{h} {label}")
        finally:
            pt.Dispose()


@pytest.mark.parametrize("size", [1, 2, 5])
def test_sky_ties_equal_the_oracle(native_builder, oracle_mod, size):
    """8 x 8 frames of one ray each straight into a sky of 1, 2 and 5 texels per face: along every axis, along (1, 1, 0) (two components bit-equal: the face ties of SampleSky),
    along (1, 1, 1) and (-1, 1, 1)"""
    sc = A.cached_room("sky_probe", native_builder, size)
    for cid, s, d in A.sky_cases():
        if s != size:
            continue
        pf = A.parallel_camera((0.0, 0.0, 0.0), d)
        for label, options, ov, frames, batch in A.VARIANTS:
            o = _oracle(oracle_mod, (cid, (8, 8), A.settings_key(ov, {}, frames)), sc, pf, 8, 8, ov, frames)
            pt = _gpu(sc, pf, 8, 8, options, ov, frames, batch)
            try:
                _hold(pt, o, sc, 8, f"{cid} {label}")
            finally:
                pt.Dispose()


@pytest.mark.parametrize("frame", A.FRAMES, ids=[f"{w}x{h}" for w, h in A.FRAMES])
def test_non_finite_frames_equal_the_oracle_up_to_nan_payloads(native_builder, oracle_mod, frame):
    """An emission that overflows to +inf and throughputs of exactly 0, two accumulated frames: the image holds inf, then inf * 0.  The one relaxed comparison of this file
    (A.same_value): positions of NaNs and signed infinities must match, finite values compare on bits.  x86 and the device produce default NaNs of opposite sign."""
    w, h = frame
    sc = A.cached_room("non_finite", native_builder); pf = A.camera("A", w, h)
    for label, options, ov, frames, batch in A.VARIANTS:
        frames = max(frames, 2)
        o = _oracle(oracle_mod, ("non_finite", frame, A.settings_key(ov, {}, frames)), sc, pf, w, h, ov, frames)
        pt = _gpu(sc, pf, w, h, options, ov, frames, batch)
        try:
            want = A.snapshot(o); got = A.snapshot(pt)
            if ov.get("RayDepth", 7) > 1:                                   # (RayDepth 1 ends before the bounce that multiplies inf by 0)
                assert np.isinf(want["image"]).any() and np.isnan(want["image"]).any(), label
            diff = A.first_difference(got, want, sc, w, relaxed=True)
            assert diff is None, f"non_finite {w}x{h} {label}: {diff}"
        finally:
            pt.Dispose()


@pytest.mark.parametrize("sample", A.TIE_SAMPLES, ids=[f"sample{s}" for s in A.TIE_SAMPLES])
def test_draws_that_equal_the_chance_equal_the_oracle(native_builder, oracle_mod, sample):
    """`metallic > rnd`, `metallic + transmission > rnd` and `rnd01 > p` with the draw EQUAL to the chance: a 2^-24 event per hit, so the frames are planted — camera A, 64 x 64, one
    BLAS, at the sample indices (idkptSetSampleSequence) that A.find_ties found; the reference test proves with the branch record that each holds such a tie."""
    w, h = 64, 64
    sc = A.cached_room("one", native_builder); pf = A.camera("A", w, h)
    for label, options, ov, frames, batch in A.VARIANTS:
        if frames != 1 or ov.get("SamplesPerPixel", 1) != 1:
            continue                                                       # (one sample of the planted index)
        o = _oracle(oracle_mod, ("tie", sample, A.settings_key(ov, {}, 1)), sc, pf, w, h, ov, 1, sequence=sample)
        pt = _gpu(sc, pf, w, h, options, ov, 1, batch, sequence=sample)
        try:
            _hold(pt, o, sc, w, f"tie sample {sample} {label}")
        finally:
            pt.Dispose()


# ---------------------------------------------------------------------------------------------------------------- the shadow kernel
SHADOW_RUNS = [(A.SHADOW_TARGET, 1, 0), (A.SHADOW_TARGET, 4, 2 ** 24 + 1), (A.SHADOW_TARGET, 16, 0xFFFFFFFE), (A.SHADOW_BLOCKER, 4, 0xFFFFFFFE), (A.SHADOW_BLOCKER, 16, 0), (A.SHADOW_BLOCKER, 1, 2 ** 24 + 1)]


@pytest.mark.parametrize("use_tlas", [0, 1])
@pytest.mark.parametrize("frame", A.FRAMES, ids=[f"{w}x{h}" for w, h in A.FRAMES])
def test_shadows_equal_the_oracle(native_builder, oracle_mod, frame, use_tlas):
    """idkptTraceShadows == oracle.trace_shadows bit for bit on the instanced swatch room with the scaled and the mirrored instance (A.shadow_room): occluders whose alpha comes
    from a texture under every wrap mode, five blend layers (the advance-and-shorten loop and its `< 0.01` exit), an occluder at alpha == cutoff, a second light between fragment
    and target, fragments inside the target's sphere and at distance == radius, planted depth-1 pixels (output kept: pre-filled with -3), normals facing away from and
    perpendicular to the light; RayTracingSamples 1, 4, 16 and NoiseIndex 0, 2^24 + 1, 0xFFFFFFFE (the `+ 1u` wraps inside the loop).  RayTracingSamples 0 is left out:
    include/idkpt.h admits only >= 1.  One run goes through idkptTraceShadowsDevice and equals the host-pointer call."""
    import torch
    from idkengine_amd.pathtracer import PathTracer
    w, h = frame
    sc = A.shadow_room(native_builder)
    pt = PathTracer(8, 8); pt.UploadScene(sc); pt.UseTlas = use_tlas
    try:
        plain = A.cached_room("inst_x", native_builder)            # the G-buffer is an input: made on the CPU from the room without the occluders (A.shadow_gbuffer)
        cam, depth, normal, planted = A.shadow_gbuffer(sc, w, h, lambda r: oracle_mod.trace_rays(plain, r, use_tlas=bool(use_tlas)), raster=plain)
        assert (depth[0] == 1.0).all() and all(n >= 8 for _, n in planted.values()), planted
        away = planted["away"][0]
        seen = set()
        for k, (light, samples, noise) in enumerate(SHADOW_RUNS):
            p = T.ShadowParams.make(cam.inv_proj_view, w, h, light_index=light, samples=samples, noise_index=noise, jitter=(0.0005, -0.0003))
            keep = np.full((h, w), np.float32(-3.0))
            got = pt.TraceShadows(p, depth, normal, visibility=keep)
            want = oracle_mod.trace_shadows(sc, p, depth, normal, visibility=keep, use_tlas=bool(use_tlas))
            bad = np.argwhere(bits(got) != bits(want))
            assert len(bad) == 0, f"light {light} samples {samples} noise {noise}: pixel ({bad[0][1]}, {bad[0][0]}) is {got[tuple(bad[0])]!r}, the oracle has {want[tuple(bad[0])]!r}; {len(bad)} pixels differ"
            assert (got[0] == -3.0).all() and (got[away][depth[away] < 1.0] == 0.0).all()        # depth 1: kept; normals facing away: 0
            seen |= set(np.unique(got[1:]).tolist())
            if k == 1:
                dev = torch.device("cuda", 0)
                d_depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).to(dev); d_normal = torch.from_numpy(np.ascontiguousarray(normal, np.float32)).to(dev)
                d_vis = torch.from_numpy(keep.copy()).to(dev)
                torch.cuda.synchronize()
                pt.TraceShadowsDevice(p, d_depth.data_ptr(), d_normal.data_ptr(), d_vis.data_ptr())
                pt.synchronize()
                assert (bits(d_vis.cpu().numpy()) == bits(got)).all()
        assert 0.0 in seen and 1.0 in seen and len(seen) > 4                                          # lit, shadowed and partly visible (blend layers, several samples); tests/test_adversarial_surfaces_ref.py proves per occluder that shadow rays cross it
    finally:
        pt.Dispose()
