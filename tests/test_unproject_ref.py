"""The reference material of the equirectangular-sky tests, checked on the CPU: tests/unproject_ref.py (the numpy restatement of SkyBoxManager.LoadSkyBoxEquirectangular
and Shaders/UnprojectEquirectangular/compute.glsl in binary32 and in binary64) against tests/golden/unproject/cases.npz (the reference's own shader on Mesa llvmpipe,
minted by tests/golden/make_unproject.py: the uploaded texture's half bits, the floats imageStore receives, the cube's half bits, cube lookups), and the per-texel functions
the device kernels call (idkengine_amd/csrc/unproject_texel.hpp) compiled for the host under ASan/UBSan (tests/c_driver/unproject_host.cpp) against the restatement.

The tolerance the device is held to (tests/test_gpu_unproject.py) is MEASURED here, not chosen — the rule of the sky, display and bloom passes.  Per case, from the SAME
half input texels (the fixture's uploaded texture), with T the binary64 evaluation and err(X) = max |X - T| / scale over the compared texels and channels, scale = the
binary64 SrgbToLinear of the largest |tap| of the texel's four taps (alpha: the tap), at least one half subnormal: b = 2 x max(err(llvmpipe's floats), err(restatement))
(case_bound).  A stored half h passes if rtz(T - b scale) <= h <= rtz(T + b scale).  The figures are in profiles/sky_unproject.md.

Three facts of the reference on llvmpipe shape the tests:
 * llvmpipe's upload rounds to nearest even when the source has THREE channels (the reference's only path: ImageLoader.Load(path, RGB, true)) and toward zero when it has
   FOUR (Mesa packs RGBA floats by another routine).  Both are asserted on every texel.  The library's one rule is the three-channel one (a host's alpha must not change
   the colours: three channels and four with alpha 1 give identical bits); the shader stage of the four-channel case is still compared from the fixture's own texels.
 * With S = W / 4 no ordinary texel's footprint crosses an edge of the panorama (unproject_ref.wrapping_texels): REPEAT and CLAMP_TO_EDGE differ at seam texels only, so
   the clamped variant CANNOT fail on case 1 (even S, no seam texel) — asserted.  It fails on the seam-adjacent texels of the odd cases and on case 7
   (16 x 8, S = 12 > W / 4), which is where the tests tell the two apart.
 * atan(0, 0) (the centres of +-Y) is undefined in GLSL; Mesa returns +-3 pi / 4, C +-0.  The accepted branches there are the multiples of pi / 4."""
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import unproject_ref as R  # noqa: E402


def _live():
    from oracle.glref import glref as G
    return G.available()


live = pytest.mark.skipif(not _live(), reason="needs the reference's shaders and Mesa llvmpipe (build container only)")


def case_bound(fx, c):
    """(b, e_gl, e_np, evaluations) of case c from the fixture's uploaded texels; seam texels are left out of the measurement"""
    S = R.CASES[c][2]
    bits = fx[f"pano_bits_{c}"]
    ev = R.evaluate64(bits, S)
    T, scale = ev[0]
    m = R.seam_mask(S)
    e_gl = R.scaled_err(fx[f"store_f32_{c}"], T, scale, m)
    e_np = R.scaled_err(R.unproject(bits, S, np.float32)[0], T, scale, m)
    return 2.0 * max(e_gl, e_np), e_gl, e_np, ev


def within_any(h_bits, ev, b, S):
    """per texel and channel: inside rtz(T -+ b scale) of the C branch, or — seam texels only — of any allowed branch"""
    ok = R.halves_within(h_bits, ev[0][0], ev[0][1], b)
    m = R.seam_mask(S)
    for T, scale in ev[1:]:
        ok |= R.halves_within(h_bits, T, scale, b) & m[..., None]
    return ok


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


@pytest.fixture(scope="module")
def bounds(fixture):
    return [case_bound(fixture, c) for c in range(len(R.CASES))]


def test_cases_and_the_inputs_hold_what_they_must(fixture):
    assert R.CASES[:6] == ((16, 8, 4, 3, 0), (20, 10, 5, 3, 0), (18, 9, 4, 3, 0), (24, 16, 6, 3, 0), (32, 16, 9, 3, 9), (64, 32, 16, 4, 0))
    assert (fixture["cases"] == np.array(R.CASES, np.int32)).all()
    for c, (W, H, S, ch, arg) in enumerate(R.CASES):
        assert S == (arg if arg else W // 4)
        img = R.input_image(R.CASES[c])
        assert img.shape == (H, W, ch) and img.dtype == np.float32 and np.isfinite(img).all()
        rgb = img[..., :3]
        h = rgb.astype(np.float16).astype(np.float32)
        tie = (rgb != h) & (np.abs(rgb - h) * 2 == np.spacing(np.abs(h).astype(np.float16)).astype(np.float32)) & (np.abs(rgb) > 6.2e-5)
        assert (rgb == 0).any() and (rgb == np.float32(0.04045)).any() and ((rgb > 0.03) & (rgb < 0.04045)).any() and ((rgb > 0.04045) & (rgb < 0.05)).any()
        assert ((rgb < 0) & (rgb > -0.01)).any() and ((rgb > 0) & (rgb < 6.1e-5)).any() and tie.any() and rgb.max() > 3e4 and rgb.max() <= 6e4
        assert fixture[f"pano_bits_{c}"].shape == (H, W, 4) and fixture[f"cube_bits_{c}"].shape == (6, S, S, 4) and fixture[f"store_f32_{c}"].shape == (6, S, S, 4)


def test_upload_rounding_rule_holds_on_every_fixture_texel(fixture):
    """Three channels (what the reference uploads): round to nearest even, subnormal halves produced, alpha 1.0 — no exception.  Four channels: llvmpipe truncates."""
    saw_sub = saw_tie = False
    for c, case in enumerate(R.CASES):
        img = R.input_image(case); bits = fixture[f"pano_bits_{c}"]
        if case[3] == 3:
            assert (bits == R.pack(img)).all(), c
            assert (bits[..., 3] == 0x3C00).all()
            rgb = bits[..., :3]
            saw_sub |= bool((((rgb & 0x7C00) == 0) & ((rgb & 0x3FF) != 0)).any())
            saw_tie |= bool((R.rne_half(img) != R.rtz_half(img)).any())
        else:
            assert (bits == R.rtz_half(img)).all(), c
            assert (R.pack(img) != bits).any()                  # (the library's rule is NOT llvmpipe's four-channel one)
    assert saw_sub and saw_tie


def test_store_rounding_rule_holds_on_every_fixture_texel(fixture):
    """imageStore to the RGBA16F cube: toward zero, subnormals produced, 65504 beyond — bloom's rule, re-pinned on this shader"""
    differs = saturated = False
    for c in range(len(R.CASES)):
        f32, bits = fixture[f"store_f32_{c}"], fixture[f"cube_bits_{c}"]
        assert np.isfinite(f32).all()
        assert (bits == R.rtz_half(f32)).all(), c
        with np.errstate(over="ignore"):
            differs |= bool((bits != f32.astype(np.float16).view(np.uint16)).any())
        saturated |= bool(((f32 > 65504) & (bits == 0x7BFF)).any())
    assert differs and saturated


def test_seam_texels_are_few_and_only_at_odd_sizes():
    for W, H, S, ch, arg in R.CASES:
        column, poles = R.seam_masks(S)
        n = int((column | poles).sum())
        if S % 2 == 0:
            assert n == 0
        else:
            assert n == S + 2 and n <= S + 2 and int(column.sum()) == S and column[1, :, S // 2].all() and poles[2, S // 2, S // 2] and poles[3, S // 2, S // 2]


def test_fixture_and_restatement_are_within_the_measured_bound(fixture, bounds):
    for c, (W, H, S, ch, arg) in enumerate(R.CASES):
        b, e_gl, e_np, ev = bounds[c]
        m = R.seam_mask(S)
        print(f"case {c + 1} ({W} x {H}, S = {S}, {ch} channels): e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  b = {b:.3e}  seam texels {int(m.sum())}")
        assert 0 < b < 0.05, (c, b)                               # (a bound of several per cent would mean one of the two executions is not this formula)
        ok = within_any(fixture[f"cube_bits_{c}"], ev, b, S)
        assert ok.all(), (c, int((~ok).sum()))
        n32 = R.unproject(fixture[f"pano_bits_{c}"], S, np.float32)[0]
        ok = within_any(R.rtz_half(n32), ev, b, S)
        assert ok.all(), (c, int((~ok).sum()))


def test_filter_is_repeat_wrapped_not_clamped(fixture, bounds):
    told_apart = 0
    for c, (W, H, S, ch, arg) in enumerate(R.CASES):
        b, _, _, ev = bounds[c]
        bits = fixture[f"pano_bits_{c}"]
        wrapping = R.wrapping_texels(W, H, S); seam = R.seam_mask(S)
        Tc, bigc = R.unproject(bits, S, np.float64, wrap="clamp")
        fail = ~R.halves_within(fixture[f"cube_bits_{c}"], Tc, R.scale_of(bigc), b).all(axis=-1) & ~seam
        assert not (fail & ~wrapping).any()                      # (where no footprint wraps the two variants are the same formula)
        if arg == 0:
            assert not (wrapping & ~seam & ~_seam_rows(S)).any(), c   # S = W / 4: only texels with z == 0, x <= 0 wrap
        if c == 0:
            assert not wrapping.any() and not fail.any()         # case 1 cannot tell the variants apart (module docstring)
        if (wrapping & ~seam).any():
            assert fail.any(), c
            told_apart += 1
    assert told_apart >= 3                                       # cases 2, 5 and 7
    c = len(R.CASES) - 1
    W, H, S = R.CASES[c][:3]
    Tc, bigc = R.unproject(fixture[f"pano_bits_{c}"], S, np.float64, wrap="clamp")
    fail = ~R.halves_within(fixture[f"cube_bits_{c}"], Tc, R.scale_of(bigc), bounds[c][0]).all(axis=-1)
    u, v = R.spherical_uv(R.directions(S, np.float64), np.float64)
    x_wrap = (u * W - 0.5 < 0) | (u * W - 0.5 >= W - 1); y_wrap = (v * H - 0.5 < 0) | (v * H - 0.5 >= H - 1)
    assert (fail & x_wrap & ~y_wrap).any() and (fail & y_wrap & ~x_wrap).any()   # both axes


def _seam_rows(S):
    """the left half of the centre row of +-Y: z == +-0, x < 0 (unproject_ref.seam_masks)"""
    d = R.directions(S, np.float32)
    m = (d[..., 2] == 0) & (d[..., 0] < 0)
    m[1] = False
    return m


def test_cube_lookups_tie_the_resident_form_to_sample_sky(fixture):
    """texture(samplerCube, dir) on the reference's finished seamless cube against the arithmetic of SampleSky (csrc/pt_kernels.hpp) on the expanded halves.  Tolerance,
    reasoned: llvmpipe evaluates the coordinates and weights in binary32; a coordinate carries a few ulp (division by the major axis, scale, bias), which S <= 5
    multiplies into the weight — below 2^-20 per axis — and three lerps of taps no larger than M add a few ulp of M: 2^-18 M covers it with room, M the largest |tap|."""
    for c in (0, 1):
        faces = R.half_values(fixture[f"cube_bits_{c}"], np.float64)
        dirs = fixture[f"cube_dirs_{c}"]
        got = fixture[f"cube_samples_{c}"].astype(np.float64)[:, :3]
        want, big = R.sample_cube(faces, dirs)
        assert len(dirs) >= 200 and np.isfinite(got).all()
        assert (np.abs(got - want) <= 2.0 ** -18 * big[:, None]).all(), (c, float((np.abs(got - want) / big[:, None]).max()))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/unproject_host.cpp + csrc/unproject_texel.hpp under ASan and UBSan, as a stand-alone program"""
    exe = str(tmp_path_factory.mktemp("unproject_host") / "unproject_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           os.path.join(HERE, "c_driver", "unproject_host.cpp"), "-o", exe])
    return exe


def run_host_program(exe, tmp, case, img, uv, store):
    W, H, S, ch, _ = case
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([W, H, ch, S, len(uv), store.size], np.int32).tobytes())
        f.write(np.ascontiguousarray(img, np.float32).tobytes()); f.write(np.ascontiguousarray(uv, np.float32).tobytes()); f.write(np.ascontiguousarray(store, np.float32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    raw = open(dst, "rb").read()
    at = 0
    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at); at += a.nbytes
        return a
    out = dict(pano=take(np.uint16, W * H * 4).reshape(H, W, 4), value=take(np.float32, 6 * S * S * 4).reshape(6, S, S, 4), cube=take(np.uint16, 6 * S * S * 4).reshape(6, S, S, 4))
    rec = take(np.dtype([("i", np.int32, 4), ("a", np.float32, 2)]), len(uv))
    out["idx"], out["w"] = rec["i"], rec["a"]
    out["store"] = take(np.uint16, store.size)
    assert at == len(raw)
    return out


def test_host_build_of_the_kernels_texel_functions(host_program, tmp_path, fixture, bounds):
    """Bit for bit in everything without a transcendental (pack, wrap, weights, half store); inside b end to end."""
    for c, case in enumerate(R.CASES):
        W, H, S, ch, _ = case
        img = R.input_image(case)
        u, v = R.spherical_uv(R.directions(S, np.float32), np.float32)
        extra = np.array([[0.0, 1.0], [1.0, 0.0], [-0.25, 1.25], [0.5 / W, 0.5 / H], [0.99983, 0.99999], [np.float32(0.5) / np.float32(W) - np.float32(1e-7), 0.00017]], np.float32)
        uv = np.concatenate([np.stack([u.ravel(), v.ravel()], axis=1), extra]).astype(np.float32)
        store = fixture[f"store_f32_{c}"].ravel()
        got = run_host_program(host_program, str(tmp_path), case, img, uv, store)
        assert got["pano"].tobytes() == R.pack(img).tobytes(), c
        x0, x1, ax = R.taps(uv[:, 0], W, np.float32); y0, y1, ay = R.taps(uv[:, 1], H, np.float32)
        assert (got["idx"] == np.stack([x0, x1, y0, y1], axis=1)).all(), c
        assert got["w"].tobytes() == np.stack([ax, ay], axis=1).astype(np.float32).tobytes(), c
        assert (got["store"] == R.rtz_half(store)).all() and (got["store"].reshape(6, S, S, 4) == fixture[f"cube_bits_{c}"]).all(), c
        assert (got["cube"] == R.rtz_half(got["value"])).all(), c
        # end to end: from the library's own packed texels (the fixture's for three channels), inside the case's measured bound
        ev = R.evaluate64(R.pack(img), S)
        ok = within_any(got["cube"], ev, bounds[c][0], S)
        assert ok.all(), (c, int((~ok).sum()))
        m = R.seam_mask(S)
        print(f"case {c + 1}: host build err = {R.scaled_err(got['value'], ev[0][0], ev[0][1], m):.3e} (b = {bounds[c][0]:.3e}); halves differing from the restatement's: "
              f"{int((got['cube'] != R.rtz_half(R.unproject(R.pack(img), S, np.float32)[0])).sum())} of {got['cube'].size}")
        # C's signed zeros at the seam texels: +pi in the centre column of -X, 0 at the centres of +-Y — the first (numpy / C) evaluation, without any other branch
        if m.any():
            ok = R.halves_within(got["cube"], ev[0][0], ev[0][1], bounds[c][0])
            assert ok[m].all(), c


def test_library_rule_beyond_65504_saturates():
    """not compared with the reference: a finite input whose nearest half would be infinite is stored as +-65504"""
    v = np.array([65504.0, 65519.996, 65520.0, 7e4, 3e38, -65520.0, -1e9], np.float32)
    assert (R.rne_half(v) == np.array([0x7BFF] * 5 + [0xFBFF] * 2, np.uint16)).all()
    assert (R.rne_half(np.array([65519.996], np.float32)) == 0x7BFF).all() and np.float16(np.float32(65519.996)) == np.float16(65504)


@live
def test_live_fixture_is_reproducible():
    """Runs the reference's shader on llvmpipe again and demands the committed fixture bit for bit (separate process: Mesa brings its own LLVM)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_unproject.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
