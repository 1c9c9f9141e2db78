"""idkptReprojectMoments and idkptDenoiseTemporal on the CPU: tests/denoise_temporal_ref.py (the numpy binary32 restatement of the contract in include/idkpt.h, "temporal
moments") against hand-computed cases and the properties the first state has to have, and against the per-pixel functions the device kernels call
(idkengine_amd/csrc/denoise_temporal_texel.hpp, csrc/reproject_texel.hpp) compiled for the host under ASan/UBSan as a stand-alone program
(tests/c_driver/denoise_temporal_host.cpp), bit for bit.  The host program's fetches abort when they are asked for a texel outside the image, so every run also checks
that no tap is fetched unchecked."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import denoise_temporal_ref as R  # noqa: E402
import denoise_variance_ref as V  # noqa: E402
import reproject_ref as P  # noqa: E402
import test_reproject_ref as TR  # noqa: E402  (analytic_records: synthetic geometry images, inputs only)

F = np.float32
NAMES = ["idkptReprojectMoments", "idkptDownloadTemporalMoments", "idkptGetTemporalMomentsDevicePtr", "idkptDenoiseTemporal"]
FIELDS = ["Iterations", "LumaSigma", "VarianceEpsilon", "AlbedoSigma", "NormalSigma", "DemodulateAlbedo", "SpatialBelow"]


# ---- the feature exists
def test_the_library_declares_and_exports_the_entry_points():
    from idkengine_amd import _lib, gputypes as T
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.idkptGetAbiVersion() >= 12                  # (the entry points came without a new number: a host detects them by symbol)
    d = T.DenoiseTemporal()
    assert C.sizeof(T.DenoiseTemporal) == 28
    assert (d.Iterations, d.LumaSigma, d.VarianceEpsilon, d.AlbedoSigma, d.NormalSigma, d.DemodulateAlbedo, d.SpatialBelow) == (5, 1.0, F(0.1), F(0.2), 0.5, 1, 4.0)
    assert R.DEFAULTS == dict(Iterations=5, LumaSigma=1.0, VarianceEpsilon=0.1, AlbedoSigma=0.2, NormalSigma=0.5, DemodulateAlbedo=1, SpatialBelow=4.0)
    # without a device the calls refuse a NULL context like every other entry point
    assert L.idkptDenoiseTemporal(None, 0, None) == 2 and L.idkptReprojectMoments(None, 0, -2, None) == 2
    assert L.idkptDownloadTemporalMoments(None, 0, None, 0) == 2 and L.idkptGetTemporalMomentsDevicePtr(None, 0, None, None) == 2
    from idkengine_amd.pathtracer import PathTracer
    for m in ("ReprojectMoments", "DownloadTemporalMoments", "temporal_moments_device_ptr", "DenoiseTemporal"):
        assert callable(getattr(PathTracer, m))
    # enum idkpt_denoise_input did not grow
    assert (T.IDKPT_DENOISE_INPUT_ACCUMULATED, T.IDKPT_DENOISE_INPUT_TEMPORAL) == (0, 1)


def test_struct_layout_matches_the_header(tmp_path):
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idkpt.h"\nint main(void){printf("%zu ' + "%zu " * len(FIELDS) + '%d\\n", sizeof(idkpt_denoise_temporal), '
                 + ", ".join(f"offsetof(idkpt_denoise_temporal, {f})" for f in FIELDS) + ', IDKPT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    from idkengine_amd import gputypes as T, _lib
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got[:8] == [C.sizeof(T.DenoiseTemporal)] + [getattr(T.DenoiseTemporal, f).offset for f in FIELDS]
    assert got[:8] == [28, 0, 4, 8, 12, 16, 20, 24]
    assert got[8] == _lib.load().idkptGetAbiVersion()     # the header's number is the library's: the section came under the current one


# ---- the shared inputs show what they must show (on the CPU, from the restatement alone)
def test_the_synthetic_counts_straddle_the_threshold():
    assert sorted({c[:2] for c in R.CASES}) == sorted(R.SHAPES) == sorted([(1, 1), (3, 5), (16, 16), (17, 16), (37, 29), (64, 48)])
    for shape in R.SHAPES:
        assert {(s["Iterations"], s["DemodulateAlbedo"]) for w, h, s in R.CASES if (w, h) == shape} == {(i, d) for i in (1, 2, 5) for d in (0, 1)}
    assert {V.route(i) for i in range(5)} == {V.ROUTE_TILED, V.ROUTE_DIRECT} and [1 << i for i in range(5) if V.route(i) == V.ROUTE_DIRECT] == [8, 16]
    for W, H in R.SHAPES:
        images = R.random_images(W, H)
        br = {}
        c0, v0 = R.first_state(*images, SpatialBelow=4.0, branch=br)
        assert not br["nonfinite"].any() and np.isfinite(v0).all()
        if W * H > 15:
            assert br["temporal"].mean() >= 0.1 and br["spatial"].mean() >= 0.1, (W, H, br["temporal"].mean(), br["spatial"].mean())
            assert (images[1][..., 3] == 4.0).any() and br["temporal"][images[1][..., 3] == 4.0].all()      # cnt == SpatialBelow: the temporal branch
            assert (v0 == 0).any() and (v0 > 1e-3).any()


# ---- hand-computed cases
def flat_guides(H, W):
    a = np.full((H, W, 4), 0.5, F); n = np.zeros((H, W, 4), F); n[..., 2] = 1.0
    return a, n


def test_the_first_state_by_hand():
    H, W = 1, 4
    a, n = flat_guides(H, W)
    t = np.ones((H, W, 4), F)
    tm = np.zeros((H, W, 4), F)
    tm[0, :, 0] = 0.5; tm[0, :, 1] = (0.75, 0.5, 0.25, 0.75); tm[0, :, 3] = (5.0, 1.0, 2.0, 4.0)
    br = {}
    c0, v0 = R.first_state(t, tm, a, n, DemodulateAlbedo=0, branch=br)
    assert br["temporal"].tolist() == [[True, False, False, True]] and (c0 == 1.0).all()
    assert v0[0, 0] == F(0.5) / F(4.0) and v0[0, 3] == F(0.5) / F(3.0)           # (0.75 - 0.25) / (cnt - 1)
    # flat guides: every weight is 1; pixel 1 sees all four texels (dx -1 .. 2), a1 = 0.5, a2 = (0.75 + 0.5 + 0.25 + 0.75) / 4 = 0.5625: (0.5625 - 0.25) / cnt
    assert (br["sW"] == 4.0).all()
    assert v0[0, 1] == F(0.3125) / F(1.0) and v0[0, 2] == F(0.3125) / F(2.0)
    c0, v1 = R.first_state(t, tm, a, n, DemodulateAlbedo=1)
    assert (c0 == 2.0).all() and R.same(v1, v0 / F(0.25))                          # lum(0.5, 0.5, 0.5) = 0.5 exactly
    # a guide edge takes the other side's moments out of the estimate by its weight: w = 1 / (1 + 3 * 0.25 / 0.04) across the albedo step
    a[0, 2:, :3] = 1.0
    _, v2 = R.first_state(t, tm, a, n, DemodulateAlbedo=0, branch=br)
    w = F(1.0) / (F(1.0) + F(F(0.25) + F(0.25) + F(0.25)) * V.inv_sigma2(0.2))
    assert br["sW"][0, 1] == (F(1.0) + F(1.0)) + w + w


def test_the_history_start_and_a_pixel_that_finds_itself():
    cur, g, hg, hc = TR.tiny()
    mom = np.zeros_like(cur); mom[..., 0] = cur[..., 0]; mom[..., 1] = cur[..., 1] + 1.0; mom[..., 3] = 1.0
    hm = hc.copy(); hm[..., 2] = 123.0                                           # whatever the history held in z: the output stores 0
    assert R.same(R.start_moments(mom, 3)[..., :2], mom[..., :2]) and (R.start_moments(mom, 3)[..., 2] == 0).all() and (R.start_moments(mom, 3)[..., 3] == 3.0).all()
    out = R.reproject_moments(mom, 2, g, hg, hm, TR.IDENT, (0, 0, 5))
    n = F(2.0)
    for (y, x) in [(0, 0), (3, 3), (1, 2)]:
        Hc = hm[y, x, 3]
        want = [F(F(F(hm[y, x, k] * Hc) + F(mom[y, x, k] * n)) / F(Hc + n)) for k in range(2)] + [F(0.0), F(Hc + n)]
        assert R.same(out[y, x], np.array(want, F))
    # the alpha is the colour reprojection's, bit for bit (the metamorphic relation of the GPU test)
    hc2 = hc.copy(); hc2[..., 3] = hm[..., 3]
    assert R.same(out[..., 3], P.reproject(cur, 2, g, hg, hc2, TR.IDENT, (0, 0, 5))[..., 3])
    # a non-finite channel of the history texel, z included, invalidates the tap
    hm[1, 2, 2] = np.inf
    assert R.same(R.reproject_moments(mom, 2, g, hg, hm, TR.IDENT, (0, 0, 5))[1, 2], np.array([mom[1, 2, 0], mom[1, 2, 1], 0.0, 2.0], F))


# ---- the host build of the kernels' per-pixel functions
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/denoise_temporal_host.cpp + the two texel headers under ASan and UBSan, as a stand-alone program"""
    return R.build_host_program(str(tmp_path_factory.mktemp("denoise_temporal_host") / "denoise_temporal_host"))


def differing(got, want):
    return int((R.bits(got) != R.bits(want)).any(axis=2).sum())


def test_host_build_of_the_filter_equals_the_restatement_bit_for_bit(host_program, tmp_path):
    for W, H, s in R.CASES:
        images = R.random_images(W, H)
        got, want = R.host_filter(host_program, str(tmp_path), images, s), R.denoise_temporal(*images, **s)
        assert R.same(got, want), (W, H, s, differing(got, want))
    images = R.random_images(37, 29, seed=1)
    for s in (dict(R.DEFAULTS), R.settings(3, 1, SpatialBelow=2.0), R.settings(3, 0, SpatialBelow=100.0)):       # the defaults; nearly all temporal; all spatial
        got, want = R.host_filter(host_program, str(tmp_path), images, s), R.denoise_temporal(*images, **s)
        assert R.same(got, want), (s, differing(got, want))


def test_host_build_equals_the_restatement_on_the_plants_and_they_stay_where_they_are(host_program, tmp_path):
    W, H = R.PLANT_SHAPE
    clean = R.random_images(W, H)
    for pname, writes in R.PLANTS:
        for pos in R.PLANT_POSITIONS:
            x, y = pos
            images = R.plant(clean, writes, pos)
            br = {}
            _, v0 = R.first_state(*images, DemodulateAlbedo=0, branch=br)
            if writes[0][0] != R.TEMPORAL:
                assert not np.isfinite(v0[y, x]), (pname, pos)                   # a moment, a count or every weight not finite; cnt = 0 divides by 0
            if "spatial pixel" in pname:
                assert br["spatial"][y, x] and br["sW"][y, x] == 0 and np.isposinf(v0[y, x])
            if pname.startswith(("M1", "M2", "cnt=nan", "cnt=+inf", "cnt=-inf")):
                assert br["nonfinite"][y, x] and np.isposinf(v0[y, x])
            others = np.ones((H, W), bool); others[y, x] = False
            for s in R.PLANT_SETTINGS:
                got, want = R.host_filter(host_program, str(tmp_path), images, s), R.denoise_temporal(*images, **s)
                assert R.same(got, want), (pname, pos, s, differing(got, want))
                assert np.isfinite(want[others]).all(), (pname, pos, s)          # nothing spreads
                if not s["DemodulateAlbedo"] and writes[0][0] != R.NORMAL and writes[0][0] != R.ALBEDO:
                    assert R.same(want[y, x, :3], images[0][y, x, :3]), (pname, pos)      # the planted pixel keeps its temporal rgb


def test_host_build_of_the_moments_reprojection_equals_the_restatement(host_program, tmp_path):
    from idkengine_amd import scenes as S
    W, H = 37, 23
    rng = np.random.default_rng(5)
    prev = S.Camera(W, H, position=(0.2, 0.1, 2.0), view_dir=(0.0, 0.0, -1.0), fovy_deg=80.0)
    hg = P.pack(*TR.analytic_records(prev, W, H))
    M = (prev.view @ prev.proj).astype(F)
    seen = {k: 0 for k in ("clip_w", "offscreen", "id", "position", "colour", "history")}
    for mv in (dict(position=(0.25, 0.1, 2.0), view_dir=(0.05, 0.0, -1.0)), dict(position=(1.5, 0.4, 1.0), view_dir=(-0.6, 0.0, -1.0)), dict(position=(0.2, 0.1, -8.0), view_dir=(0.0, 0.0, 1.0))):
        g = P.pack(*TR.analytic_records(S.Camera(W, H, fovy_deg=80.0, **mv), W, H))
        mom = rng.random((H, W, 4)).astype(F); mom[..., 2] = 0.0; mom[..., 3] = 1.0
        hm = (rng.random((H, W, 4)) * 2.0).astype(F); hm[..., 2] = 0.0; hm[..., 3] = rng.integers(1, 60, (H, W)).astype(F)
        hm[5, 7, 0] = np.nan; hm[9, 20, 3] = np.inf; hm[14, 30, 2] = -np.inf; hm[3, 3, 2] = 7.0       # invalid taps, and a finite z that must not reach the output
        for n, s in ((1, {}), (3, dict(PositionTolerance=1e-3, MaxHistory=8.0))):
            st = {}
            want = R.reproject_moments(mom, n, g, hg, hm, M, prev.position, stats=st, **s)
            got = R.host_moments(host_program, str(tmp_path), mom, n, g, hg, hm, M, prev.position, **s)
            assert R.same(got, want), differing(got, want)
            assert (want[..., 2] == 0).all() and (R.bits(want[..., 2]) == 0).all()
            assert R.same(want[~st["history"]], R.start_moments(mom, n)[~st["history"]])
            for k in seen:
                seen[k] += int(st[k].sum())
        start = R.host_moments(host_program, str(tmp_path), mom, 2, g, hg, hm, M, prev.position, start=True)
        assert R.same(start, R.start_moments(mom, 2))
    assert all(v > 0 for v in seen.values()), seen


# ---- the point of it: the variance follows the history
def test_a_short_history_is_filtered_harder_than_a_long_one():
    """the same noisy luminance step under flat guides: where the count is high the variance of the mean is small and the edge-stopping kernel keeps the step, where the
    history is one sample the spatial estimate is large and the step is smoothed"""
    H, W = 16, 32
    rng = np.random.default_rng(3)
    a, n = flat_guides(H, W)
    t = np.full((H, W, 4), 0.5, F); t[:, W // 2:, :3] += F(0.25)
    tm = np.zeros((H, W, 4), F)
    L = V.lum(t[..., :3])
    per_sample = F(0.04)
    tm[..., 0] = L; tm[..., 1] = L * L + per_sample
    step = lambda im: float(im[:, W // 2, 0].astype(np.float64).mean() - im[:, W // 2 - 1, 0].astype(np.float64).mean())
    out = {}
    for cnt in (1.0, 32.0):
        tm[..., 3] = cnt
        out[cnt] = R.denoise_temporal(t, tm, a, n, **dict(R.DEFAULTS, DemodulateAlbedo=0, VarianceEpsilon=1e-4))
    assert step(out[32.0]) > step(out[1.0]) > 0.0, (step(out[32.0]), step(out[1.0]))
