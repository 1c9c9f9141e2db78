"""The reference material of the bloom tests, checked on the CPU: tests/bloom_ref.py (the numpy restatement of Shaders/Bloom/compute.glsl as Bloom.cs drives it, binary32
operation for operation, and the same formula in binary64) against tests/golden/bloom/chain.npz (the reference's own shader on Mesa llvmpipe, minted by
tests/golden/make_bloom.py: per pass the value imageStore receives and the bits of the R16G16B16A16Float level), and the per-texel functions the device kernels call
(idkengine_amd/csrc/bloom_texel.hpp) compiled for the host under ASan/UBSan (tests/c_driver/bloom_host.cpp) against the restatement bit for bit.

The tolerance the device is held to (tests/test_gpu_bloom.py) is MEASURED here, not chosen — the rule of the sky and of the display pass.  GLSL leaves the arithmetic of
the linear filter to the implementation, so two correct binary32 executions differ.  Per case and pass, from the SAME input bits (the fixture's previous levels), with T
the binary64 evaluation and err(X) = max |X - T| over R, G, B: e_gl = err(llvmpipe's floats), e_np = err(restatement); a third execution can land on the other side of T
from either, hence b = 2 x max(e_gl, e_np) (pass_bound).  A stored half h passes if rtz(T - b) <= h <= rtz(T + b) (halves_within).  Where both executions are exact
(powers of two as weights on short sums) b is 0 and the half must be rtz(T)."""
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import bloom_ref as R  # noqa: E402


def _live():
    from oracle.glref import glref as G
    return G.available()


live = pytest.mark.skipif(not _live(), reason="needs the reference's shaders and Mesa llvmpipe (build container only)")


def pass_bound(fx_f32, np32, np64):
    """(b, e_gl, e_np) of one pass"""
    e_gl, e_np = R.err(fx_f32, np64), R.err(np32, np64)
    return 2.0 * max(e_gl, e_np), e_gl, e_np


def halves_within(bits, v64, b):
    """rtz(v64 - b) <= h <= rtz(v64 + b), per R, G, B, compared as values"""
    h = R.half_values(np.asarray(bits)[..., :3], np.float64)
    lo = R.half_values(R.rtz_half(v64 - b), np.float64); hi = R.half_values(R.rtz_half(v64 + b), np.float64)
    return (lo <= h) & (h <= hi)


def evaluate_passes(fx, c):
    """[(name, chain, level, fixture bits, fixture floats, binary32 restatement, binary64 evaluation)] of case c in the order Bloom.Compute runs the passes; every pass is
    evaluated from the fixture's own input bits."""
    case = R.CASES[c]
    W, H, thr, maxc, minus = case
    levels, sz = R.sizes(W, H, minus)
    img = R.input_image(case)
    out = []
    for l in range(levels):
        ev = (lambda dt: R.down_pass0(img, sz[0], thr, maxc, dt)) if l == 0 else (lambda dt, l=l: R.down_pass(fx[f"down_bits_{c}_{l - 1}"], sz[l], dt, (thr, maxc) if l == 1 else None))
        out.append((f"down {l}", "down", l, fx[f"down_bits_{c}_{l}"], fx[f"down_f32_{c}_{l}"], ev(np.float32), ev(np.float64)))
    for l in range(levels - 2, -1, -1):
        a = fx[f"down_bits_{c}_{l + 1}"] if l == levels - 2 else fx[f"up_bits_{c}_{l + 1}"]
        ev = lambda dt, a=a, l=l: R.up_pass(a, fx[f"down_bits_{c}_{l + 1}"], sz[l], dt)
        out.append((f"up {l}", "up", l, fx[f"up_bits_{c}_{l}"], fx[f"up_f32_{c}_{l}"], ev(np.float32), ev(np.float64)))
    return out


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.fixture(scope="module")
def evaluated(fixture):
    return [evaluate_passes(fixture, c) for c in range(len(R.CASES))]


def test_cases_are_the_issues_and_sizes_follow_bloom_cs(fixture):
    assert [c[:2] for c in R.CASES] == [(64, 48), (37, 23), (40, 6), (2, 2), (261, 141)]
    assert R.CASES[2][4] == 0 and R.CASES[4][2:] == (1.5, 3.8, 3) and (fixture["cases"] == np.array(R.CASES, np.float32)).all()
    # Bloom.SetSize: integer division, GetMaxMipmapLevel = floor(log2(max)) + 1, minus MinusLods, at least 2; level l = max(d >> l, 1)
    assert R.sizes(1920, 1080, 3) == (7, [(960, 540), (480, 270), (240, 135), (120, 67), (60, 33), (30, 16), (15, 8)])
    assert R.sizes(3840, 2160, 3)[0] == 8 and R.sizes(37, 23, 3) == (2, [(18, 11), (9, 5)]) and R.sizes(2, 2, 3) == (2, [(1, 1), (1, 1)]) and R.sizes(3, 3, 0) == (2, [(1, 1), (1, 1)])
    assert R.sizes(40, 6, 0) == (5, [(20, 3), (10, 1), (5, 1), (2, 1), (1, 1)]) and R.sizes(64, 48, 3)[0] == 3 and R.sizes(261, 141, 3)[0] == 5
    # the fixture's level shapes are the sizes GL gave the mip levels
    for c, case in enumerate(R.CASES):
        levels, sz = R.sizes(case[0], case[1], case[4])
        for l in range(levels):
            assert fixture[f"down_bits_{c}_{l}"].shape == (sz[l][1], sz[l][0], 4) and fixture[f"down_f32_{c}_{l}"].shape == (sz[l][1], sz[l][0], 4)
        for l in range(levels - 1):
            assert fixture[f"up_bits_{c}_{l}"].shape == (sz[l][1], sz[l][0], 4)
        assert f"down_bits_{c}_{levels}" not in fixture.files and f"up_bits_{c}_{levels - 1}" not in fixture.files
        assert fixture[f"expand_{c}"].shape == (case[1], case[0], 4)


def test_inputs_cover_what_the_issue_lists(fixture):
    for c, case in enumerate(R.CASES):
        img = R.input_image(case)
        assert img.shape == (case[1], case[0], 4) and img.dtype == np.float32 and np.isfinite(img).all()
    sub = lambda b: ((((b[..., :3] >> 10) & 31) == 0) & ((b[..., :3] & 0x3FF) != 0)).any()
    for c in (1, 4):                                   # the default settings
        W, H, thr, maxc, _ = R.CASES[c]
        img = R.input_image(R.CASES[c]); b = img[..., :3].max(axis=-1)
        assert (img[..., :3] == 0).all(axis=-1).any() and (b < thr - R.KNEE).any() and ((b > thr - R.KNEE) & (b < thr + R.KNEE)).any() and (b > thr + R.KNEE).any() and (b > maxc).any()
        assert sub(fixture[f"down_bits_{c}_0"]) and sub(fixture[f"up_bits_{c}_0"])            # values that land on half subnormals
        assert (fixture[f"up_bits_{c}_0"][..., :3] != 0).any()                                  # something survives both prefilters
    # the case whose levels exceed 65504: saturating stores in both chains, and floats beyond 65504 in front of them
    assert (fixture["down_bits_0_0"][..., :3] == 0x7BFF).any() and (fixture["up_bits_0_0"][..., :3] == 0x7BFF).any() and fixture["down_f32_0_0"][..., :3].max() > 65504.0
    assert np.isfinite(fixture["down_f32_0_0"]).all()


def test_reference_halves_follow_the_headers_rounding_with_no_exception(fixture, evaluated):
    """On EVERY texel of the fixture llvmpipe's RGBA16F bits are the header's rule (toward zero, 65504 on overflow, subnormals) applied to llvmpipe's own floats; alpha is 1."""
    texels = 0
    for passes in evaluated:
        for name, chain, l, bits, f32, _, _ in passes:
            assert bits.dtype == np.uint16 and f32.dtype == np.float32 and (bits[..., 3] == 0x3C00).all() and (f32[..., 3] == 1.0).all()
            assert (R.store(f32[..., :3]) == bits).all(), name
            texels += bits.shape[0] * bits.shape[1]
    assert texels > 25000
    # ... and round-to-nearest would not reproduce them
    f32 = fixture["down_f32_4_0"][..., :3]
    assert (f32.astype(np.float16).view(np.uint16) != fixture["down_bits_4_0"][..., :3]).any()


def test_rtz_half_is_the_headers_rule():
    v = np.array([0.0, 1.0, 1.0009765625, np.float32(1.0009765625) - np.float32(2.0 ** -23), 1.00146484375, -1.00146484375, 65504.0, 65519.0, 65520.0, 65536.0, 70000.0, 3e38, -70000.0,
                  6.103515625e-5, 6.1e-5, 5.9604644775390625e-8, 1.1e-7, 5.9e-8, 1e-30, -1.5e-7], np.float32)
    want = [0x0000, 0x3C00, 0x3C01, 0x3C00, 0x3C01, 0xBC01, 0x7BFF, 0x7BFF, 0x7BFF, 0x7BFF, 0x7BFF, 0x7BFF, 0xFBFF, 0x0400, 0x03FF, 0x0001, 0x0001, 0x0000, 0x0000, 0x8002]
    assert R.rtz_half(v).tolist() == want and R.rtz_half(v.astype(np.float64)).tolist() == want
    assert R.rtz_half(np.array([1.0 + 2.0 ** -10 - 2.0 ** -40])).tolist() == [0x3C00]           # binary64 just below the next half
    every = np.arange(0x10000, dtype=np.uint32).astype(np.uint16); every = every[((every >> 10) & 31) != 31]
    assert (R.rtz_half(R.half_values(every, np.float32)) == every).all()


def test_every_pass_of_both_binary32_executions_sits_inside_the_bound(evaluated):
    for c, passes in enumerate(evaluated):
        for name, chain, l, bits, f32, np32, np64 in passes:
            b, e_gl, e_np = pass_bound(f32, np32, np64)
            scale = float(np.abs(np64).max())
            print(f"case {c} {name} {bits.shape[1]}x{bits.shape[0]}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {b:.3e}  (largest value {scale:.4g})  restatement == llvmpipe's floats bit for bit on "
                  f"{float((f32[..., :3].view(np.uint32) == np32.view(np.uint32)).mean()):.3f} of the values; its halves on {float((R.store(np32)[..., :3] == bits[..., :3]).mean()):.4f}")
            assert np32.dtype == np.float32 and np64.dtype == np.float64 and np.isfinite(np64).all()
            assert b <= 2.0 ** -12 * scale                                    # a quarter of a half step of the pass's largest value (the filter weights of an odd size carry the rounding of a coordinate near `size`: 2^-24 size x the texel range); beyond it the restatement is not the shader
            assert halves_within(bits, np64, b).all() and halves_within(R.store(np32), np64, b).all()


def test_expand_of_both_binary32_executions_sits_inside_the_bound(fixture):
    for c, case in enumerate(R.CASES):
        up0 = fixture[f"up_bits_{c}_0"]
        e32, e64 = R.expand(up0, case[0], case[1], np.float32), R.expand(up0, case[0], case[1], np.float64)
        fx = fixture[f"expand_{c}"]
        b, e_gl, e_np = pass_bound(fx, e32, e64)
        print(f"case {c} expand {case[0]}x{case[1]}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {b:.3e}")
        assert (fx[..., 3] == 1.0).all() and b <= 2.0 ** -12 * float(e64.max())
        assert R.err(fx, e64) <= b and R.err(e32, e64) <= b


def test_whole_chain_from_the_image_matches_the_fixture_within_the_bound(fixture, evaluated):
    """The restatement's chain from the IMAGE (its own half storage at every level) against the binary64 chain with the same storage rule: the per-pass bound applies to
    the values in front of every store (what the GPU test does with the device's levels)."""
    for c, case in enumerate(R.CASES):
        c32, c64 = R.chain(R.input_image(case), case, np.float32), R.chain(R.input_image(case), case, np.float64)
        for name, chain, l, bits, f32, np32, np64 in evaluated[c]:
            b, _, _ = pass_bound(f32, np32, np64)
            ok = halves_within(c32[chain][l], c64[chain + "_f"][l], b)
            steps = np.abs(c32[chain][l][..., :3].astype(np.int64) - c64[chain][l][..., :3].astype(np.int64))          # (all values are >= 0: bit patterns are ordered)
            print(f"case {c} {name}: restatement chain halves outside rtz(T -+ b): {int((~ok).sum())} of {ok.size}; largest distance from the binary64 chain's half: {int(steps.max())} step(s); "
                  f"differing from llvmpipe's bits: {int((c32[chain][l] != bits).sum())}")
            # The whole-chain rule.  The per-pass bound holds wherever both chains fed the pass the same bits; behind a level where a store flipped (the binary32 value
            # and the binary64 value on different sides of a half) the inputs differ by one step, b (4e-16 where a pass is exact) no longer covers it, and what holds
            # instead is the distance in steps: every pass is a sum with positive weights of non-negative halves, so inputs one step apart move the output by about
            # one step of ITS size, and the next store truncates it again.  Measured on this fixture (profiles/bloom.md): never more than 1 step at any level of any
            # case, and outside rtz(T -+ b) only in the up levels of case 4 — both are asserted, so a chain that drifts further fails here.
            assert steps.max() <= 1, (c, name, int(steps.max()))
            if not (c == 4 and chain == "up"):
                assert ok.all(), (c, name, int((~ok).sum()))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/bloom_host.cpp + csrc/bloom_texel.hpp under ASan and UBSan, as a stand-alone program"""
    exe = str(tmp_path_factory.mktemp("bloom_host") / "bloom_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           os.path.join(HERE, "c_driver", "bloom_host.cpp"), "-o", exe])
    return exe


def run_host_program(exe, tmp, case, img):
    W, H, thr, maxc, minus = case
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([W, H, minus], np.int32).tobytes()); f.write(np.array([thr, maxc], np.float32).tobytes()); f.write(np.ascontiguousarray(img, np.float32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    raw = open(dst, "rb").read()
    levels, sz = R.sizes(W, H, minus)
    assert np.frombuffer(raw[:4], np.int32)[0] == levels
    at = 4; out = dict(down=[], up=[])
    for chain, n in (("down", levels), ("up", levels - 1)):
        for l in range(n):
            nb = sz[l][0] * sz[l][1] * 8
            out[chain].append(np.frombuffer(raw[at:at + nb], np.uint16).reshape(sz[l][1], sz[l][0], 4)); at += nb
    out["expand"] = np.frombuffer(raw[at:], np.float32).reshape(H, W, 4)
    return out


def test_host_build_of_the_kernels_texel_functions_equals_the_restatement_bit_for_bit(host_program, tmp_path):
    for c, case in enumerate(R.CASES):
        img = R.input_image(case)
        got = run_host_program(host_program, str(tmp_path), case, img)
        want = R.chain(img, case, np.float32)
        for chain in ("down", "up"):
            assert len(got[chain]) == len(want[chain])
            for l, (g, w) in enumerate(zip(got[chain], want[chain])):
                assert g.tobytes() == w.tobytes(), (c, chain, l, int((g != w).sum()))
        assert got["expand"][..., :3].tobytes() == np.ascontiguousarray(want["expand"]).tobytes() and (got["expand"][..., 3] == 1.0).all(), c


@live
def test_live_fixture_is_reproducible():
    """Runs the reference's shader on llvmpipe again and demands the committed fixture bit for bit (separate process: Mesa brings its own LLVM)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_bloom.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
