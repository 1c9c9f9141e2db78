"""The reference material of the display tests, checked on the CPU: tests/present_ref.py (the numpy restatement of Shaders/TonemapAndGammaCorrect/compute.glsl, binary32
operation for operation, and the same formula in binary64) against tests/golden/present/agx.npz (the reference's own shader on Mesa llvmpipe, minted by
tests/golden/make_present.py: the value imageStore receives, and the bytes of its R8G8B8A8Unorm image).

The tolerance the device is held to (tests/test_gpu_present.py) is MEASURED here, not chosen — the sky's rule (tests/test_sky_ref.py).  GLSL leaves inverse(mat3), exp, pow,
the association of a matrix product and the contraction of a * b + c to the implementation, so two correct binary32 executions differ.  With T the binary64 evaluation and
err(X) = max |X - T| over R, G, B (absolute: the output lives in [0, 1]), the two binary32 executions we have give e_gl = err(fixture) and e_np = err(restatement) per case;
a third execution can land on the other side of T from either, hence the bound 2 x max(e_gl, e_np) of the same case (present_bound below; the figures are recorded in
profiles/present.md).  The bound has to stay below half a byte step, 1 / 510: above it the 8-bit image would not be determined by the formula."""
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import present_ref as R  # noqa: E402


def _live():
    from oracle.glref import glref as G
    return G.available()


live = pytest.mark.skipif(not _live(), reason="needs the reference's shaders and Mesa llvmpipe (build container only)")


@pytest.fixture(scope="module")
def evaluated():
    """[(case, fixture floats, fixture bytes, binary32 restatement, binary64 evaluation)], computed once."""
    out = []
    for case, fx, by in R.load_fixture():
        img, add = R.case_inputs(case)
        out.append((case, fx, by, R.present(img, case, add, None, np.float32), R.present(img, case, add, None, np.float64)))
    return out


def present_bound(fx, f32, f64):
    """(bound, e_gl, e_np) of one case: what a further binary32 execution — the device — may differ from the binary64 value by."""
    e_gl, e_np = R.err(fx, f64), R.err(f32, f64)
    return 2.0 * max(e_gl, e_np), e_gl, e_np


def test_fixture_holds_the_cases_of_the_issue(evaluated):
    assert len(evaluated) == len(R.CASES) == 10
    for (case, fx, by, _, _), want in zip(evaluated, R.CASES):
        assert all(np.float32(a) == np.float32(b) for a, b in zip(case[:5], want[:5])) and case[5:] == want[5:]
        assert fx.dtype == np.float32 and fx.shape == (R.H, R.W, 4) and np.isfinite(fx).all()
        assert by.dtype == np.uint8 and by.shape == (R.H, R.W, 4)
    c = [tuple(float(np.float32(v)) for v in k[:5]) + k[5:] for k in R.CASES]
    f = lambda *v: tuple(float(np.float32(x)) for x in v)
    assert c[0] == f(0.45, 1.06, 0.18, 1.0, 0.1) + (1, 0) and c[1][5] == 0 and c[9][6] == 1
    assert {k[0] for k in c} >= set(f(-2.0, 3.0)) and {k[1] for k in c} >= set(f(0.0, 1.5)) and {k[4] for k in c} >= set(f(0.0, 0.4)) and f(0.5, 0.8) in {k[2:4] for k in c}
    # the input: 70 x 40 (width = 2 mod 4 and no multiple of 8; five bands of 8 rows), exact zero, negative components, values up to 1e4, finite
    img = R.input_image()
    assert img.shape == (40, 70, 4) and img.dtype == np.float32 and np.isfinite(img).all()
    assert (img[..., :3] == 0).any() and (img[..., :3] < 0).any() and img.max() == np.float32(1e4)
    # dense ramps across the DualSection joint (in the adjusted space: sRGB_to_adjusted * colour * 2^Exposure against Peak * Linear) and across the sRGB cutoff (in the
    # encoded value: 12.92 * 0.0031308) of the default settings: texels on both sides within 2 % of either
    m, minv, e2 = R.matrices(R.DEFAULTS, np.float64)
    rgb = np.maximum(img[..., :3].astype(np.float64), 0.0) * float(e2)
    adjusted = np.stack(R._mul_mv(m, [rgb[..., 0], rgb[..., 1], rgb[..., 2]]), -1)
    xs = np.arange(R.W) % 8; ys = np.arange(R.H) % 8
    encoded = evaluated[0][4][..., :3] - R.dither_values(np.float64)[xs[None, :], ys[:, None]][..., None]
    for v, joint in ((adjusted, 0.18), (encoded, 12.92 * 0.0031308)):
        assert ((v > joint * 0.98) & (v < joint)).any() and ((v > joint) & (v < joint * 1.02)).any(), joint


def test_both_binary32_executions_sit_inside_the_bound(evaluated):
    for k, (case, fx, by, f32, f64) in enumerate(evaluated):
        bound, e_gl, e_np = present_bound(fx, f32, f64)
        print(f"case {k} {case}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {bound:.3e}  (half a byte step: {1 / 510:.3e})  texels equal bit for bit: {float((fx.view(np.uint32) == f32.view(np.uint32)).all(-1).mean()):.3f}")
        assert f32.dtype == np.float32 and f64.dtype == np.float64
        assert e_gl <= bound and e_np <= bound                       # (by construction)
        assert 0.0 < bound < 1.0 / 510.0, (k, bound)                 # the 8-bit image is determined by the formula; if not, the INPUTS are wrong
        for im in (fx, f32, f64):
            assert (im[..., 3] == 1.0).all()


def test_reference_bytes_follow_the_headers_quantisation(evaluated):
    """llvmpipe's RGBA8 image equals the header's rule applied to llvmpipe's own floats; a byte may differ only where x * 255 lies within 1e-4 of a rounding tie — and on this
    input no byte does (the exceptions are counted: there are none to excuse)."""
    exceptions = 0
    for k, (case, fx, by, _, _) in enumerate(evaluated):
        q = R.quantise(fx)
        x = np.minimum(np.maximum(fx.astype(np.float64), 0.0), 1.0) * 255.0
        near_tie = np.abs((x - np.floor(x)) - 0.5) < 1e-4
        diff = q != by
        assert (by[..., 3] == 255).all()
        assert not (diff[..., :3] & ~near_tie[..., :3]).any(), k
        exceptions += int(diff.sum())
    assert exceptions == 0


def test_dither_is_the_shaders_table_indexed_x_first():
    d = R.dither_values(np.float32)
    assert d.dtype == np.float32 and d[1, 0] == (np.float32(33.0) / np.float32(65.0) - np.float32(0.5)) / np.float32(64.0) and d[0, 1] == (np.float32(49.0) / np.float32(65.0) - np.float32(0.5)) / np.float32(64.0)
    assert sorted(R.BAYER.ravel().tolist()) == list(range(1, 65)) and not (R.BAYER == R.BAYER.T).all()
    grey = np.full((16, 16, 4), 0.5, np.float32)
    out = R.present(grey, R.DEFAULTS[:5] + (0,), dtype=np.float32)
    for y in range(16):
        for x in range(16):
            assert out[y, x, 0] == np.float32(0.5) + d[x % 8, y % 8]
    # rows of the whole frame: a shard that starts at row 3 continues the pattern
    assert R.present(grey[3:], R.DEFAULTS[:5] + (0,), dtype=np.float32, first_row=3).tobytes() == out[3:].tobytes()


def test_quantise_is_round_to_nearest_even_with_alpha_255():
    x = np.array([[-1.0, 0.0, 2.0, 0.25], [1.0, 0.999, 0.5, 0.75], [0.00196, 0.00197, 0.3, 0.0]], np.float32)
    q = R.quantise(x)
    want = [[int(round(float(np.float32(min(max(float(v), 0.0), 1.0)) * np.float32(255.0)))) for v in row[:3]] + [255] for row in x]     # (Python's round: ties to even, like rintf)
    assert q.dtype == np.uint8 and q.tolist() == want and q[0].tolist() == [0, 0, 255, 255] and q[1, 2] == 128                # 0.5 * 255 = 127.5: the tie goes to the even 128
    assert np.rint(np.float32(0.5)) == 0 and np.rint(np.float32(1.5)) == 2 and np.rint(np.float32(2.5)) == 2


def test_matrices_follow_the_shader():
    """sRGB_to_adjusted is the identity at Compression 0 (adjusted_to_XYZ is sRGB_to_XYZ then), its inverse is its inverse, and the product is taken in the shader's WRITTEN
    order sRGB_to_XYZ * XYZ_to_adjusted (GLSL: the right factor acts first) — the other order would keep white white, this one does not, and llvmpipe agrees (the fixture)."""
    for comp in (0.0, 0.1, 0.4):
        m, minv, e2 = R.matrices((0.45, 1.06, 0.18, 1.0, comp, 1), np.float64)
        M = np.array(m).T; Mi = np.array(minv).T            # m[c][r] -> rows
        assert np.allclose(M @ Mi, np.eye(3), atol=1e-12)
        if comp == 0.0:
            assert np.allclose(M, np.eye(3), atol=1e-12)
        else:
            f = np.float64
            xyz = np.array(R._primaries_to_matrix([f(0.64), f(0.33)], [f(0.3), f(0.6)], [f(0.15), f(0.06)], [f(0.3127), f(0.3290)], f)).T
            adj = np.linalg.inv(xyz) @ M                    # M = xyz @ inverse(adjusted_to_XYZ)  ->  inverse(adjusted_to_XYZ)
            assert np.allclose((np.linalg.inv(adj) @ np.ones(3)), xyz @ np.ones(3), atol=1e-9)     # adjusted white = D65 = sRGB white, in XYZ
            assert not np.allclose(M.sum(axis=1), 1.0, atol=1e-3)
        assert abs(e2 - 2.0 ** float(np.float32(0.45))) < 1e-15


@live
def test_live_fixture_is_reproducible():
    """Runs the reference's shader on llvmpipe again and demands the committed fixture bit for bit (separate process: Mesa brings its own LLVM)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_present.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
