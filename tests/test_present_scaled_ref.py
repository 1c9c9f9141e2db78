"""The reference material of the presentation-size tests (idkptSetPresentationSize), checked on the CPU: tests/present_scaled_ref.py (the numpy restatement: the GL 4.6
8.14.2 linear filter of tests/bloom_ref.py, then tests/present_ref.py / tests/bloom_ref.py) against tests/golden/present_scaled/*.npz (the reference's own tonemap and
bloom shaders on Mesa llvmpipe with Sampler0 at the render size and ImgResult / the chain at the presentation size; tests/golden/make_present_scaled.py), and the host build
of the filter and texel functions the device calls (tests/c_driver/present_scaled_host.cpp under ASan / UBSan) against the restatement bit for bit.

Tolerances are measured, not chosen — the rule of tests/test_present_ref.py: per case bound = 2 x max(e_gl, e_np) against the binary64 evaluation, and for a present case
0 < bound < 1 / 510 (half a byte step; a condition on the INPUTS).  Measured on this fixture: bounds 3.5e-7 ... 2.9e-4 (profiles/present_scaled.md).

What "bit for bit" can cover.  The tone curve uses exp and pow, and no two libraries agree on them: numpy's binary32 np.exp / np.power differ from glibc's expf / powf on
40 % / 18 % of 200 000 random arguments (measured when this was written), and the device's differ from both (profiles/present.md: 2-7 % of texels equal).  So, as for the
unscaled display (tests/test_gpu_present.py), values BEHIND the tone curve are held to the bound, and bit-for-bit equality is demanded of everything IN FRONT of it — the
filtered sum ((0 + texture(Sampler0, uv)) + s1) + s2, which is all the scaled path adds — and of the whole display where the curve is off (DoTonemapAndSrgbTransform = 0:
clamp and dither, single correctly rounded operations), for every fixture size, and of every bloom level and the expanded image."""
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bloom_ref as B  # noqa: E402
import present_ref as P  # noqa: E402
import present_scaled_ref as R  # noqa: E402


def _live():
    from oracle.glref import glref as G
    return G.available()


live = pytest.mark.skipif(not _live(), reason="needs the reference's shaders and Mesa llvmpipe (build container only)")


@pytest.fixture(scope="module")
def evaluated():
    """[(key, (pw, ph), case, rows, fixture floats, fixture bytes, binary32 restatement, binary64 evaluation)] of cases.npz, computed once"""
    fx = np.load(R.FIXTURE)
    out = []
    for key, img, (pw, ph), c in R.entries():
        case, add = P.CASES[c], R.case_add(c, pw, ph)
        rows, f, b = R.fixture_entry(fx, key, pw, ph)
        out.append((key, (pw, ph), case, rows, f, b, R.present_scaled(img, pw, ph, case, add, None, np.float32), R.present_scaled(img, pw, ph, case, add, None, np.float64)))
    assert sorted(fx.files) == sorted(["float_" + e[0] for e in out] + ["bytes_" + e[0] for e in out])
    return out


@pytest.fixture(scope="module")
def bloom_fx():
    return np.load(R.BLOOM_FIXTURE)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("present_scaled_host")
    return R.build_host(d), d


def test_fixture_holds_the_sizes_and_cases_of_the_issue(evaluated, bloom_fx):
    assert R.SIZES == ((93, 53), (140, 80), (700, 400), (71, 41), (35, 20), (23, 13)) and R.CASE_IDS == (0, 1, 9) and R.SMALL == ((3, 2), (9, 7))
    assert (P.W, P.H) == (70, 40) and P.CASES[1][5] == 0 and P.CASES[9][6] == 1 and P.CASES[0] == P.DEFAULTS + (0,)
    keys = [e[0] for e in evaluated]
    for (pw, ph) in R.SIZES:
        assert f"{pw}x{ph}_0" in keys and ((pw, ph) == R.BIG or (f"{pw}x{ph}_1" in keys and f"{pw}x{ph}_9" in keys))
    assert {"small_0", "small_1", "small_9"} <= set(keys) and R.small_image().shape == (2, 3, 4)
    assert sorted(set(int(r) % 8 for r in R.BIG_ROWS)) == list(range(8))
    assert {pw % 4 for pw, _ in R.SIZES} == {0, 1, 3} | ({2} & {pw % 4 for pw, _ in R.SIZES})
    assert R.BLOOM_CHAINS == ((70, 40, 93, 53), (70, 40, 140, 80), (70, 40, 23, 13), (3, 2, 2, 2)) and (bloom_fx["chains"] == np.array(R.BLOOM_CHAINS)).all()
    for c, (W, H, pw, ph) in enumerate(R.BLOOM_CHAINS):
        levels, sz = B.sizes(pw, ph, R.BLOOM_SETTINGS[2])                       # the chain is sized from the PRESENTATION size
        for l in range(levels):
            assert bloom_fx[f"down_bits_{c}_{l}"].shape == (sz[l][1], sz[l][0], 4)
        assert f"down_bits_{c}_{levels}" not in bloom_fx.files and bloom_fx[f"expand_{c}"].shape == (ph, pw, 4)
        assert R.bloom_source(W, H).shape == (H, W, 4)
    assert (bloom_fx["up_bits_0_0"][..., :3] != 0).any() and (bloom_fx["up_bits_2_0"][..., :3] != 0).any()      # something survives both prefilters


def test_both_binary32_executions_sit_inside_the_bound(evaluated):
    for key, size, case, rows, fx, by, f32, f64 in evaluated:
        bound, e_gl, e_np = R.bound_of(fx, f32[rows], f64[rows])
        e_np_all = P.err(f32, f64)
        bound = max(bound, 2.0 * e_np_all)
        print(f"{key}: e_gl = {e_gl:.3e}  e_np = {e_np_all:.3e}  bound = {bound:.3e}  (half a byte step: {1 / 510:.3e})")
        assert f32.dtype == np.float32 and f64.dtype == np.float64 and (fx[..., 3] == 1.0).all() and (f32[..., 3] == 1.0).all()
        assert 0.0 < bound < 1.0 / 510.0, (key, bound)                  # the 8-bit image is determined by the formula; if not, the INPUTS are wrong


def test_reference_bytes_follow_the_headers_quantisation(evaluated):
    """llvmpipe's RGBA8 ImgResult equals the header's rule applied to llvmpipe's own floats; a byte may differ only within 1e-4 of a rounding tie — counted: none does."""
    exceptions = 0
    for key, size, case, rows, fx, by, _, _ in evaluated:
        q = P.quantise(fx)
        x = np.minimum(np.maximum(fx.astype(np.float64), 0.0), 1.0) * 255.0
        near_tie = np.abs((x - np.floor(x)) - 0.5) < 1e-4
        diff = q != by
        assert (by[..., 3] == 255).all() and not (diff[..., :3] & ~near_tie[..., :3]).any(), key
        exceptions += int(diff.sum())
    assert exceptions == 0


def test_dither_is_indexed_by_the_presentation_texel():
    grey = np.full((40, 70, 4), 0.5, np.float32)
    out = R.present_scaled(grey, 93, 53, P.DEFAULTS[:5] + (0,), dtype=np.float32)
    d = P.dither_values(np.float32)
    want = np.float32(0.5) + d[(np.arange(93) % 8)[None, :], (np.arange(53) % 8)[:, None]]
    assert out.shape == (53, 93, 4) and (out[..., 0] == want).all() and (out[..., 2] == want).all()


def test_sampling_at_the_source_size_is_close_to_the_texel_fetch_but_not_it():
    """At equal sizes the filter's weight is 0 only up to rounding (a sample at a texel centre is not exactly the texel): why equal sizes keep the texel-fetch kernel."""
    img = P.input_image()
    s64, s32 = R.sample(img, P.W, P.H, np.float64), R.sample(img, P.W, P.H, np.float32)
    assert np.abs(s64 - img[..., :3]).max() <= 2.0 ** -40 * 1e4 and np.abs(s32.astype(np.float64) - img[..., :3]).max() <= 2.0 ** -16 * 1e4
    assert s32.tobytes() != img[..., :3].tobytes()


def test_bloom_halves_of_both_binary32_executions_sit_inside_the_per_pass_bound(bloom_fx):
    for c in range(len(R.BLOOM_CHAINS)):
        for name, chain, l, bits, f32, np32, np64 in R.bloom_passes(bloom_fx, c):
            b, e_gl, e_np = R.bound_of(f32, np32, np64, B.err)
            scale = float(np.abs(np64).max())
            print(f"chain {c} {name} {bits.shape[1]}x{bits.shape[0]}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {b:.3e}  (largest value {scale:.4g})")
            assert (bits[..., 3] == 0x3C00).all() and (B.store(f32[..., :3]) == bits).all()            # llvmpipe's halves are the header's rule on its own floats
            assert b <= 2.0 ** -12 * max(scale, 2.0 ** -14)
            assert R.halves_within(bits, np64, b).all() and R.halves_within(B.store(np32), np64, b).all()     # rtz(T - b) <= h <= rtz(T + b)
        W, H, pw, ph = R.BLOOM_CHAINS[c]
        up0 = bloom_fx[f"up_bits_{c}_0"]
        e32, e64 = B.expand(up0, pw, ph, np.float32), B.expand(up0, pw, ph, np.float64)
        b, _, _ = R.bound_of(bloom_fx[f"expand_{c}"], e32, e64, B.err)
        assert b <= 2.0 ** -12 * max(float(e64.max()), 2.0 ** -14) and B.err(bloom_fx[f"expand_{c}"], e64) <= b and B.err(e32, e64) <= b


def test_host_build_of_the_filter_equals_the_restatement_bit_for_bit_on_every_size(host):
    exe, d = host
    img = P.input_image()
    for (pw, ph) in R.SIZES + ((P.W, P.H),):
        for adds in ((), (R.bloom_image(pw, ph),), (R.bloom_image(pw, ph), R.bloom_image(pw, ph)[::-1].copy())):
            got = R.host_sum(exe, d, img, pw, ph, adds)
            want = R.sampled_sum(img, pw, ph, *(list(adds) + [None, None])[:2], dtype=np.float32)
            assert got.tobytes() == want.tobytes(), (pw, ph, len(adds))
        # ... and so does the whole display where the tone curve is off (CASES[1]): clamp and dither are single binary32 operations
        assert R.no_tonemap_display(R.host_sum(exe, d, img, pw, ph)).tobytes() == R.present_scaled(img, pw, ph, P.CASES[1], dtype=np.float32).tobytes()
    got = R.host_sum(exe, d, R.small_image(), *R.SMALL[1])
    assert got.tobytes() == R.sampled_sum(R.small_image(), *R.SMALL[1], dtype=np.float32).tobytes()


def test_filter_is_exact_under_power_of_two_scales_and_sign(host):
    """What lets the GPU test look at the sum in front of the clamp: host_sum(img * s) == host_sum(img) * s bit for bit for s = +-2^k (no value leaves the normal range), and
    every value of the sum of magnitude 2^-18 and above lands in [2^-4, 1] for one of them."""
    exe, d = host
    img = P.input_image()
    for (pw, ph) in ((93, 53), (23, 13)):
        base = R.host_sum(exe, d, img, pw, ph)
        seen = np.zeros(base.shape, bool)
        for k in R.SCALE_EXPONENTS:
            for sign in (1.0, -1.0):
                sc = np.float32(sign * 2.0 ** k)
                scaled = img.copy(); scaled[..., :3] *= sc
                hs = base * sc + np.float32(0.0)                         # (0 + (-0) = +0: the sum starts from the shader's 0)
                assert R.host_sum(exe, d, scaled, pw, ph).tobytes() == hs.tobytes(), (pw, ph, k, sign)
                seen |= (hs >= 2.0 ** -4) & (hs <= 1.0)
        assert (seen | (np.abs(base) < 2.0 ** -18)).all() and (base < 0).any() and base.max() > 1e3      # (below 2^-18: filter residue next to the exact zero of the input)


def test_host_build_of_the_bloom_chain_equals_the_restatement_bit_for_bit_by_both_routes(host):
    exe, d = host
    for c, (W, H, pw, ph) in enumerate(R.BLOOM_CHAINS):
        img = R.bloom_source(W, H)
        got, want = R.host_bloom(exe, d, img, pw, ph), R.bloom_chain(img, pw, ph, np.float32)
        assert got["same"] == 1, c                                       # down pass 0 through the staged tile == through clamped fetches from memory
        for chain in ("down", "up"):
            assert len(got[chain]) == len(want[chain])
            for l, (g, w) in enumerate(zip(got[chain], want[chain])):
                assert g.tobytes() == w.tobytes(), (c, chain, l)
        assert got["expand"][..., :3].tobytes() == want["expand"].tobytes() and (got["expand"][..., 3] == 1.0).all()


@live
def test_live_fixture_is_reproducible():
    """Runs the reference's shaders on llvmpipe again and demands the committed fixtures bit for bit (separate process: Mesa brings its own LLVM)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_present_scaled.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
