"""The noise estimate on the CPU: tests/noise_ref.py (the numpy binary32 restatement of the contract in include/idkpt.h) against hand-computed cases and against the
per-texel functions the device kernels call (idkengine_amd/csrc/noise_texel.hpp) compiled for the host under ASan/UBSan as a stand-alone program
(tests/c_driver/noise_host.cpp), bit for bit: the fold, the per-pixel error, the tile tree and the summary, on random inputs and on the edge cases of the contract.

Moments the fold itself produces are never -0.0 (m1 and m2 start at +0.0 and x * (1 - w) + y * w of two zeros of either sign is +0.0 unless both are negative, which
L * L never is), so fmaxf(-0.0, 0.0) — whose sign the C standard leaves open — is not among the cases."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import noise_ref as R  # noqa: E402

F = np.float32
FLT_MAX = np.finfo(F).max
SHAPES = [(24, 16), (20, 13), (8, 8), (9, 1), (1, 9), (37, 23)]           # whole tiles; tiles cut by the right and bottom edges; one tile; one row / one column of tiles


# ---- the feature exists
def test_the_library_declares_and_exports_the_noise_entry_points():
    from idkengine_amd import _lib, gputypes as T
    names = ["idkptSetNoiseEstimate", "idkptGetNoiseEstimate", "idkptEstimateNoise", "idkptDownloadNoise", "idkptGetNoiseDevicePtr", "idkptDownloadMoments", "idkptGetMomentsDevicePtr"]
    L = _lib.load()
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.idkptGetAbiVersion() >= 12                  # (the seven entry points came without a new number: a host detects them by symbol, as above)
    p = T.Noise()
    assert C.sizeof(T.Noise) == 8 and C.sizeof(T.NoiseSummary) == 16 and (p.Epsilon, p.Threshold) == (F(1e-2), F(0.05))
    assert R.DEFAULTS == dict(Epsilon=1e-2, Threshold=0.05)
    # without a device the calls refuse a NULL context like every other entry point
    assert L.idkptSetNoiseEstimate(None, 1) == 2 and L.idkptEstimateNoise(None, 0, None) == 2 and L.idkptDownloadNoise(None, 0, None, 0, None) == 2 and L.idkptDownloadMoments(None, 0, None, 0) == 2


def test_struct_layout_matches_the_header(tmp_path):
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idkpt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(idkpt_noise), offsetof(idkpt_noise, Epsilon), '
                 'offsetof(idkpt_noise, Threshold), sizeof(idkpt_noise_summary), offsetof(idkpt_noise_summary, TilesAbove), offsetof(idkpt_noise_summary, MaxTileMean), '
                 'offsetof(idkpt_noise_summary, Tiles), offsetof(idkpt_noise_summary, Samples), IDKPT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    from idkengine_amd import gputypes as T
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    S = T.NoiseSummary
    assert got == [C.sizeof(T.Noise), T.Noise.Epsilon.offset, T.Noise.Threshold.offset, C.sizeof(S), S.TilesAbove.offset, S.MaxTileMean.offset, S.Tiles.offset, S.Samples.offset, got[-1]] and got[-1] >= 12


# ---- hand-computed cases of the restatement
def test_the_fold_of_known_samples():
    # two samples whose luminance is one coefficient and zero: every product below is written out by hand
    nr = np.zeros((1, 1, 4), F)
    a = nr.copy(); a[..., 1] = 1.0                        # L = 0.7152f
    b = nr.copy()                                         # L = 0
    m1, m2 = R.moments([a, b])
    L = F(0.7152)
    assert R.same(m1, np.array([[L * F(0.5) + F(0.0)]], F)) and R.same(m2, np.array([[(L * L) * F(0.5)]], F))
    # the first sample's weight is 1: whatever finite value the slot held is gone
    m1, m2 = R.moments([a], m1=np.full((1, 1), 7.0, F), m2=np.full((1, 1), 9.0, F))
    assert R.same(m1, np.array([[L]], F)) and R.same(m2, np.array([[L * L]], F))


def test_the_pixel_error_by_hand():
    # m1 = 2, m2 = 5: var = 1; n = 5: sqrt(1 / 4) = 0.5; / (2 + 0.5) = 0.2
    assert R.same(R.pixel_error(F(2.0), F(5.0), 5, 0.5), F(0.5) / F(2.5))
    # m2 < m1 * m1 by rounding: clamped to 0
    assert R.same(R.pixel_error(F(3.0), np.nextafter(F(9.0), F(0.0)), 2, 1e-2), F(0.0))
    # a black pixel: 0 / Epsilon; a negative mean counts as 0 in the denominator only
    assert R.same(R.pixel_error(F(0.0), F(0.0), 2, 1e-2), F(0.0))
    assert R.same(R.pixel_error(F(-1.0), F(5.0), 2, 0.25), F(2.0) / F(0.25))
    for bad in (np.nan, np.inf, -np.inf):
        assert R.same(R.pixel_error(F(bad), F(1.0), 3, 1e-2), F(np.inf)) and R.same(R.pixel_error(F(1.0), F(bad), 3, 1e-2), F(np.inf))
    # FLT_MAX is finite: m1 * m1 overflows, the difference is -Inf, the clamp makes it 0
    assert R.same(R.pixel_error(F(FLT_MAX), F(FLT_MAX), 2, 1e-2), F(0.0))


def test_the_tile_tree_is_pairwise_and_cut_tiles_divide_by_their_own_count():
    # 64 values whose left-to-right sum differs from the pairwise one in binary32
    e = np.full((8, 8), F(1e-8), F); e[0, 0] = 1.0
    t = R.tile_map(e)
    left_to_right = F(0.0)
    for v in e.reshape(-1):
        left_to_right = F(left_to_right + v)
    pairwise = F(F(1.0) + F(63 * 1e-8))                    # every other partial sum is small and exact enough to be added once: by hand below
    lvl = e.reshape(-1).copy()
    for mask in (1, 2, 4, 8, 16, 32):
        lvl = lvl + lvl[np.arange(64) ^ mask]
    assert R.same(t[0, 0, 0], lvl[0] / F(64)) and not R.same(lvl[0], left_to_right) and abs(float(lvl[0]) - float(pairwise)) < 1e-6
    assert R.same(t[0, 0, 1], F(1.0))
    # 9 x 3: tile (0, 1) holds 1 x 3 pixels; its mean divides by 3, positions outside count as 0 in the tree and are no candidates of the maximum
    e = np.zeros((3, 9), F); e[:, 8] = [3.0, 6.0, 9.0]
    t = R.tile_map(e)
    assert t.shape == (1, 2, 2) and R.same(t[0, 1], np.array([6.0, 9.0], F)) and R.same(t[0, 0], np.array([0.0, 0.0], F))
    s = R.summary(t, 5.0, 4)
    assert s == {"TilesAbove": 1, "MaxTileMean": F(6.0), "Tiles": 2, "Samples": 4}
    e[1, 8] = np.inf
    t = R.tile_map(e)
    assert np.isposinf(t[0, 1]).all() and R.summary(t, 5.0, 4)["TilesAbove"] == 1 and np.isposinf(R.summary(t, 5.0, 4)["MaxTileMean"])


# ---- the host build of the kernels' per-texel functions
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/noise_host.cpp + csrc/noise_texel.hpp under ASan and UBSan, as a stand-alone program"""
    exe = str(tmp_path_factory.mktemp("noise_host") / "noise_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           os.path.join(HERE, "c_driver", "noise_host.cpp"), "-o", exe])
    return exe


def run_host_program(exe, tmp, start, samples, accumulated, n, eps, thr):
    H, W = start.shape[:2]
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([W, H, len(samples), n], np.int32).tobytes()); f.write(np.array([accumulated], np.uint32).tobytes()); f.write(np.array([eps, thr], F).tobytes())
        f.write(np.ascontiguousarray(start, F).tobytes())
        for im in samples:
            f.write(np.ascontiguousarray(im, F).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    raw = np.frombuffer(open(dst, "rb").read(), np.uint32)
    ty, tx = (H + 7) // 8, (W + 7) // 8
    mom = raw[:H * W * 4].view(F).reshape(H, W, 4); tiles = raw[H * W * 4:H * W * 4 + ty * tx * 2].view(F).reshape(ty, tx, 2); s = raw[H * W * 4 + ty * tx * 2:]
    assert s.size == 4
    return mom, tiles, {"TilesAbove": int(s[0]), "MaxTileMean": s[1:2].view(F)[0], "Tiles": int(s[2]), "Samples": int(s[3])}


def check(exe, tmp, start, samples, accumulated, n, eps, thr):
    mom, tiles, s = run_host_program(exe, tmp, start, samples, accumulated, n, eps, thr)
    m1, m2 = (start[..., 0], start[..., 1]) if not samples else R.moments(samples, start[..., 0], start[..., 1], accumulated)
    want_tiles, want_s = R.estimate(m1, m2, n, eps, thr)
    if samples:
        assert R.same(mom, R.moments_image(m1, m2))
    else:
        assert R.same(mom, start)
    assert R.same(tiles, want_tiles), int((R.bits(tiles) != R.bits(want_tiles)).sum())
    assert R.same_summary(s, want_s), (s, want_s)
    return tiles, s


def random_samples(W, H, K, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        im = np.ones((H, W, 4), F)
        im[..., :3] = (rng.random((H, W, 3)) ** 4 * 8.0).astype(F)          # mostly dark, some bright: the spread of a path tracer's samples
        im[rng.random((H, W)) < 0.2, :3] = 0.0                              # black pixels
        out.append(im)
    return out


def test_host_build_equals_the_restatement_on_random_samples(host_program, tmp_path):
    for i, (W, H) in enumerate(SHAPES):
        zero = np.zeros((H, W, 4), F)
        for K in (2, 3, 6):
            samples = random_samples(W, H, K, seed=10 * i + K)
            tiles, s = check(host_program, str(tmp_path), zero, samples, 0, K, 1e-2, 0.05)
            assert np.isfinite(tiles).all() and s["Tiles"] == ((W + 7) // 8) * ((H + 7) // 8)
        # a batch that continues an accumulation: samples 2..4 folded onto the moments of samples 0..1
        samples = random_samples(W, H, 5, seed=99 + i)
        m1, m2 = R.moments(samples[:2])
        check(host_program, str(tmp_path), R.moments_image(m1, m2), samples[2:], 2, 5, 0.5, 0.3)


def edge_moments(W, H):
    """moments images with the contract's edge cases planted, each with the pixel it sits at"""
    rng = np.random.default_rng(7)
    m1 = (rng.random((H, W)) * 2.0).astype(F)
    m2 = (m1 * m1 + (rng.random((H, W)) * 0.5).astype(F)).astype(F)
    sub = F(1e-42)                                                          # subnormal
    plants = [("var_clamped", F(3.0), np.nextafter(F(9.0), F(0.0))), ("m1_zero", F(0.0), F(0.0)), ("m1_zero_m2_pos", F(0.0), F(0.25)), ("m1_negative", F(-1.5), F(4.0)),
              ("nan_m1", F(np.nan), F(1.0)), ("nan_m2", F(1.0), F(np.nan)), ("inf_m1", F(np.inf), F(np.inf)), ("neg_inf_m1", F(-np.inf), F(1.0)), ("inf_m2", F(1.0), F(np.inf)),
              ("flt_max_both", F(FLT_MAX), F(FLT_MAX)), ("flt_max_m2", F(1.0), F(FLT_MAX)), ("flt_max_m1", F(FLT_MAX), F(1.0)), ("subnormal", sub, sub), ("subnormal_m2", F(0.0), sub)]
    return m1, m2, plants


@pytest.mark.parametrize("shape", [(24, 16), (20, 13)], ids=["24x16", "20x13"])
def test_host_build_equals_the_restatement_on_the_edge_cases(host_program, tmp_path, shape):
    W, H = shape
    m1, m2, plants = edge_moments(W, H)
    base, _ = R.estimate(m1, m2, 4, 1e-2, 0.05)
    for where in [(0, 0), (W - 1, H - 1), (W - 1, 3), (5, H - 1)]:          # a whole tile's corner; the cut tiles of the right and the bottom edge
        for name, a, b in plants:
            p1, p2 = m1.copy(), m2.copy(); p1[where[1], where[0]] = a; p2[where[1], where[0]] = b
            for n in (2, 4):                                                # n = 2: the division by (n - 1) is by 1
                tiles, s = check(host_program, str(tmp_path), R.moments_image(p1, p2), [], 0, n, 1e-2, 0.05)
                t = (where[1] // 8, where[0] // 8)
                if not (np.isfinite(a) and np.isfinite(b)):
                    assert np.isposinf(tiles[t]).all() and np.isposinf(s["MaxTileMean"]), name
                    if n == 4:
                        others = np.ones(tiles.shape[:2], bool); others[t] = False
                        assert R.same(tiles[others], base[others]), name    # no other tile changes
                else:
                    assert np.isfinite(tiles).all(), name
    # thresholds: 0 counts every tile with a positive mean, a huge one none
    _, s0 = check(host_program, str(tmp_path), R.moments_image(m1, m2), [], 0, 3, 1e-2, 0.0)
    _, s1 = check(host_program, str(tmp_path), R.moments_image(m1, m2), [], 0, 3, 1e-2, 1e30)
    assert s0["TilesAbove"] == s0["Tiles"] and s1["TilesAbove"] == 0


def test_host_build_folds_non_finite_and_extreme_radiance_as_the_restatement(host_program, tmp_path):
    W, H = 20, 13
    samples = random_samples(W, H, 4, seed=5)
    for value in (np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, 1e-42):
        planted = [s.copy() for s in samples]
        planted[1][4, 17, 0] = value                                        # in the cut tile of the right edge, in the second sample
        tiles, s = check(host_program, str(tmp_path), np.zeros((H, W, 4), F), planted, 0, 4, 1e-2, 0.05)
        if not np.isfinite(F(value)) or abs(float(F(value))) == float(FLT_MAX):
            assert np.isposinf(tiles[0, 2]).all()                           # FLT_MAX: L * L overflows, m2 is +Inf
