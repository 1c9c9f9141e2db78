"""The reference material of the sky tests, checked on the CPU: tests/sky_ref.py (the numpy restatement of Shaders/AtmosphericScattering/compute.glsl, binary32 operation
for operation, and the same formula in binary64) against tests/golden/sky/atmosphere.npz (the reference's own shader on Mesa llvmpipe, minted by tests/golden/make_sky.py).

The tolerance the device is held to (tests/test_gpu_sky.py) is MEASURED here, not chosen.  The arithmetic subtracts 6 371 000 from lengths near it: one binary32 ulp there is
0.5 m against a 1 200 m scale height, so two correct binary32 executions differ far above 1 ulp.  With T the binary64 evaluation and
err(X) = max |X - T| / (|T| + 1e-3 max T) over R, G, B, the two binary32 executions we have give e_gl = err(fixture) and e_np = err(restatement) per case; a third execution
(other exp / pow / sqrt roundings) can land on the other side of T from either, hence the bound 2 x max(e_gl, e_np) of the same case (sky_bound below; the figures
are recorded in profiles/sky_atmosphere.md).  Should the two differ by more than 10x on a case, one of them is wrong — most likely the restatement — and the bound means nothing:
that is asserted here."""
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sky_ref as R  # noqa: E402


def _live():
    from oracle.glref import glref as G
    return G.available()


live = pytest.mark.skipif(not _live(), reason="needs the reference's shaders and Mesa llvmpipe (build container only)")


@pytest.fixture(scope="module")
def evaluated():
    """[(case, fixture faces, binary32 restatement, binary64 evaluation)], computed once."""
    return [(case, fx, R.atmosphere(*case, dtype=np.float32), R.atmosphere(*case, dtype=np.float64)) for case, fx in R.load_fixture()]


def sky_bound(fx, f32, f64):
    """(bound, e_gl, e_np) of one case: what a further binary32 execution — the device — may differ from the binary64 value by."""
    e_gl, e_np = R.err(fx, f64), R.err(f32, f64)
    return 2.0 * max(e_gl, e_np), e_gl, e_np


def mirror_z(F):
    """The faces reflected across the plane z = 0 (the plane the sun lies in when Azimuth = 0): +X, -X flip their columns (x = -z / +z), +Y, -Y their rows, +Z and -Z swap
    with flipped columns (include/Math.glsl:17-39)."""
    M = np.empty_like(F)
    M[0] = F[0][:, ::-1]; M[1] = F[1][:, ::-1]; M[2] = F[2][::-1]; M[3] = F[3][::-1]; M[4] = F[5][:, ::-1]; M[5] = F[4][:, ::-1]
    return M


def test_fixture_holds_the_cases_of_the_issue(evaluated):
    assert len(evaluated) == 5
    for (case, fx, _, _), want in zip(evaluated, R.CASES):
        assert case[:3] == want[:3] and np.float32(case[3]) == np.float32(want[3]) and np.float32(case[4]) == np.float32(want[4]) and np.float32(case[5]) == np.float32(want[5])
        assert fx.dtype == np.float32 and fx.shape == (6, case[0], case[0], 4) and np.isfinite(fx).all()
    assert [c[0] for c in R.CASES] == [8, 5, 8, 4, 8]


def test_restatement_against_the_reference_shader(evaluated):
    for k, (case, fx, f32, f64) in enumerate(evaluated):
        bound, e_gl, e_np = sky_bound(fx, f32, f64)
        print(f"case {k + 1} {case}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {bound:.3e}  max T = {f64[..., :3].max():.4g}")
        assert f32.dtype == np.float32 and f64.dtype == np.float64
        # the two binary32 executions agree about the size of their error (a wrong restatement would not) ...
        assert max(e_gl, e_np) <= 10.0 * min(e_gl, e_np) or max(e_gl, e_np) == 0.0, (k, e_gl, e_np)
        # ... and each is inside the bound the other sets for a further execution
        assert e_np <= 2.0 * e_gl and e_gl <= 2.0 * e_np, (k, e_gl, e_np)
        # binary32 noise, not a different formula: far below a percent, and the texels that are exactly zero (early outs, no light) agree exactly
        assert bound < 1e-2
        assert ((fx[..., :3] == 0) == (f32[..., :3] == 0)).all()


def test_alpha_is_one_and_no_light_is_exactly_zero(evaluated):
    for case, fx, f32, f64 in evaluated:
        for img in (fx, f32, f64):
            assert (img[..., 3] == 1.0).all()
    case, fx, f32, f64 = evaluated[3]
    assert case[3] == 0.0
    for img in (fx, f32, f64):
        assert (img[..., :3] == 0.0).all()


def test_faces_mirror_across_the_plane_of_the_sun(evaluated):
    """Azimuth = 0 puts the sun into the plane z = 0: the sky is its own mirror image across it.  The reflection only changes the sign of z components, whose products come
    last in every left-to-right dot product and are squared or multiplied by the sun's z = 0: exact in every precision."""
    seen = 0
    for case, fx, f32, f64 in evaluated:
        if case[4] != 0.0:
            assert not (mirror_z(f64) == f64).all()            # (the low sun at azimuth 2 is NOT symmetric: the check can fail)
            continue
        seen += 1
        for img in (fx, f32, f64):
            assert (mirror_z(img) == img).all()
    assert seen == 4


def test_directions_are_the_cube_faces():
    d = R.directions(2, np.float64)
    inv = 1.0 / np.sqrt(1.5)
    # texel (x = 0, y = 0) has ndc (-0.5, -0.5): +X -> (1, 0.5, 0.5), -Y -> (-0.5, -1, 0.5), -Z -> (0.5, 0.5, -1), normalised
    assert np.allclose(d[0, 0, 0], np.array([1.0, 0.5, 0.5]) * inv) and np.allclose(d[3, 0, 0], np.array([-0.5, -1.0, 0.5]) * inv) and np.allclose(d[5, 0, 0], np.array([0.5, 0.5, -1.0]) * inv)
    assert np.allclose(np.linalg.norm(d, axis=-1), 1.0)


def test_expanders_match_hand_computed_bytes():
    px = np.array([[10, 128, 188, 51]], np.uint8)
    # sRGB (GL 4.6 8.24): 10 / 255 <= 0.04045 -> / 12.92; 128, 188 -> ((c / 255 + 0.055) / 1.055) ^ 2.4; alpha 51 / 255 = 0.2, linear
    want = np.array([0.003035269835488375, 0.21586050011389926, 0.5028864580325687, 0.2], np.float64).astype(np.float32)
    assert R.srgb8_to_float(px).tobytes() == want.reshape(1, 4).tobytes()
    # UNORM: c / 255 in binary32
    assert R.unorm8_to_float(np.array([[0, 255, 51, 128]], np.uint8)).tobytes() == np.array([[0.0, 1.0, np.float32(51) / np.float32(255), np.float32(128) / np.float32(255)]], np.float32).tobytes()
    assert R.unorm8_to_float(px)[0, 3] == np.float32(0.2)
    assert R.srgb8_to_float(np.array([[0, 255, 0, 255]], np.uint8)).tolist() == [[0.0, 1.0, 0.0, 1.0]]


@live
def test_live_fixture_is_reproducible():
    """Runs the reference's shader on llvmpipe again and demands the committed fixture bit for bit (separate process: Mesa brings its own LLVM)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_sky.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
