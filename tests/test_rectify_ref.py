"""History rectification on the CPU: tests/rectify_ref.py (the numpy binary32 restatement of the contract in include/idkpt.h, "history rectification") against
hand-computed cases and against the per-pixel function the device kernel calls (idkengine_amd/csrc/rectify_texel.hpp) compiled for the host under ASan/UBSan as a
stand-alone program (tests/c_driver/rectify_host.cpp), bit for bit, on random images and on planted NaN, infinities, FLT_MAX and subnormals.  The host program's fetch
aborts when it is asked for a texel outside the image."""
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import rectify_ref as R  # noqa: E402

F = np.float32
NAMES = ["idkptReprojectFast", "idkptDownloadFastTemporal", "idkptGetFastTemporalDevicePtr", "idkptRectifyHistory"]
SIZES = [(1, 1), (16, 16), (17, 33), (37, 23)]                               # (W, H)


# ---- the feature exists
def test_the_library_declares_and_exports_the_rectification_entry_points(tmp_path):
    from idkengine_amd import _lib, gputypes as T
    from idkengine_amd.pathtracer import PathTracer
    import ctypes as C
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.idkptGetAbiVersion() == 13                   # (the entry points came without a new number: a host detects them by symbol)
    assert L.idkptReprojectFast(None, 0, T.IDKPT_NO_HISTORY, None) == 2 and L.idkptDownloadFastTemporal(None, 0, None, 0) == 2
    assert L.idkptGetFastTemporalDevicePtr(None, 0, None, None) == 2 and L.idkptRectifyHistory(None, 0, None) == 2
    for m in ("ReprojectFast", "RectifyHistory", "DownloadFastTemporal", "fast_temporal_device_ptr"):
        assert callable(getattr(PathTracer, m))
    d = T.Rectify()
    assert (d.Radius, d.ZLow, d.ZHigh, F(d.Epsilon)) == (2, 3.0, 6.0, F(1e-3)) and C.sizeof(d) == 16
    c = tmp_path / "e.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idkpt.h"\nint main(void){idkpt_rectify r = {2, 3.0f, 6.0f, 1e-3f};'
                 'printf("%d %zu %zu %zu %zu %d\\n", r.Radius, sizeof(r), offsetof(idkpt_rectify, ZLow), offsetof(idkpt_rectify, ZHigh), offsetof(idkpt_rectify, Epsilon), IDKPT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "e"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["2", "16", "4", "8", "12", "13"]


# ---- by hand
def flat(W, H, m, alpha_t=20.0, alpha_f=3.0):
    """one surface, t = small integers (every sum exact), f = t + m"""
    t = np.empty((H, W, 4), F); t[..., :3] = (np.arange(H * W).reshape(H, W, 1) % 7).astype(F); t[..., 3] = alpha_t
    f = t.copy(); f[..., :3] = t[..., :3] + F(m); f[..., 3] = alpha_f
    g = np.zeros((H, W, 4), F); g[..., 3] = R.asfloat(np.uint32([5]))[0]
    return t, f, g


def test_a_window_of_equal_differences_by_hand():
    # var = 0, z2 = m^2 / eps2.  Epsilon = 0.25: eps2 = 1/16; ZLow = 3, ZHigh = 6: lo2 = 9, span = 27
    s = dict(Radius=2, ZLow=3.0, ZHigh=6.0, Epsilon=0.25)
    for m, lam in ((0.5, 0.0), (1.0, None), (2.0, 1.0)):               # z2 = 4 (below), 16 (inside: lambda = 7 / 27), 64 (above)
        t, f, g = flat(9, 8, m)
        st = {}
        out = R.rectify(t, f, g, stats=st, **s)
        want = F(7.0) / F(27.0) if lam is None else F(lam)
        assert (st["lambda"] == want).all() and (st["cnt"][2:-2, 2:-2] == 25.0).all() and st["cnt"][0, 0] == 9.0
        if want == 0.0:
            assert R.same(out, t) and (st["branch"] == R.BRANCH_ZERO).all()
        else:
            assert R.same(out, (t + (f - t) * want).astype(F)) and st["blended"].all()
            assert out[0, 0, 3] == F(20.0) + F(-17.0) * want              # the count moves with the colour
    assert (st["branch"] == R.BRANCH_FULL).all() and R.same(out, f)          # lambda = 1: t + (f - t) is f where the difference is exact


def test_three_and_four_taps_at_a_corner():
    s = dict(Radius=1, ZLow=3.0, ZHigh=6.0, Epsilon=0.25)
    t, f, g = flat(6, 5, 2.0)
    st = {}
    out = R.rectify(t, f, g, stats=st, **s)
    assert st["cnt"][0, 0] == 4.0 and st["blended"][0, 0] and R.same(out[0, 0], f[0, 0])
    g[1, 1, 3] = R.asfloat(np.uint32([6]))[0]                                # the diagonal neighbour is another surface: three taps left
    out = R.rectify(t, f, g, stats=st, **s)
    assert st["cnt"][0, 0] == 3.0 and st["branch"][0, 0] == R.BRANCH_FEW and R.same(out[0, 0], t[0, 0])
    assert st["cnt"][1, 1] == 1.0 and R.same(out[1, 1], t[1, 1])             # a pixel whose id differs from all its neighbours is unchanged
    assert st["cnt"][0, 1] == 5.0 and st["blended"][0, 1]                    # (its other neighbours lose one tap and still blend)
    t1, f1, g1 = flat(1, 1, 2.0)
    assert R.same(R.rectify(t1, f1, g1, **s), t1)                            # a 1 x 1 image: one tap


# ---- the host build of the kernel's per-pixel function
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/rectify_host.cpp + csrc/rectify_texel.hpp under ASan and UBSan, as a stand-alone program"""
    return R.build_host_program(str(tmp_path_factory.mktemp("rectify_host") / "rectify_host"))


def check(exe, tmp, t, f, g, nan_class=False, **s):
    st = {}
    want = R.rectify(t, f, g, stats=st, **s)
    got, blended = R.host_rectify(exe, str(tmp), t, f, g, **s)
    eq = R.nan_same if nan_class else R.same
    assert eq(got, want), (s, int((R.bits(got) != R.bits(want)).any(axis=2).sum()))
    assert (blended == st["blended"]).all()
    return want, st


def test_host_equals_the_restatement_on_random_images(host_program, tmp_path):
    for W, H in SIZES:
        t, f, g = R.random_images(W, H, seed=100 * W + H)
        for radius in (1, 2, 3):
            out, st = check(host_program, tmp_path, t, f, g, **dict(R.DEFAULTS, Radius=radius))
            assert R.same(out[~st["blended"]], t[~st["blended"]])
    assert st["blended"].any() and (~st["blended"]).any()


def test_the_random_case_takes_every_branch():
    W, H = 37, 23
    t, f, g = R.random_images(W, H, seed=100 * W + H)
    for radius in (1, 2, 3):
        st = {}
        R.rectify(t, f, g, stats=st, **dict(R.DEFAULTS, Radius=radius))
        share = {b: float((st["branch"] == b).mean()) for b in (R.BRANCH_FEW, R.BRANCH_ZERO, R.BRANCH_RAMP, R.BRANCH_FULL)}
        assert min(share.values()) >= 0.02, (radius, share)


def test_host_equals_the_restatement_on_planted_texels(host_program, tmp_path):
    for W, H in SIZES:
        clean = R.random_images(W, H, seed=7 * W + H)
        t, f, g = R.planted(*clean, seed=W + H)
        for radius in (1, 2, 3):
            out, st = check(host_program, tmp_path, t, f, g, nan_class=True, **dict(R.DEFAULTS, Radius=radius))
            assert R.same(out[~st["blended"]], t[~st["blended"]])          # a pixel that did not blend keeps its bits, whatever they are
            assert np.isfinite(t[st["blended"]]).all() and np.isfinite(f[st["blended"]]).all()
    assert (st["branch"] == R.BRANCH_NOT_FINITE).any() and st["blended"].any()
    # the difference of two finite values overflows: the tap is dropped, and where such a pixel blends, the stored value is the infinity the text says
    t, f, g = R.uniform_change(16, 16, seed=3)
    f[5, 5, 1] = R.FLT_MAX; t[5, 5, 1] = -R.FLT_MAX
    out, st = check(host_program, tmp_path, t, f, g, **R.DEFAULTS)
    assert st["cnt"][5, 5] == 24.0 and st["blended"][5, 5] and out[5, 5, 1] == np.inf and np.isfinite(out[5, 5, [0, 2, 3]]).all()


def test_zhigh_one_ulp_above_zlow(host_program, tmp_path):
    W, H = 37, 23
    t, f, g = R.random_images(W, H, seed=5)
    lo = F(3.0); hi = np.nextafter(lo, F(np.inf))
    out, st = check(host_program, tmp_path, t, f, g, Radius=2, ZLow=float(lo), ZHigh=float(hi), Epsilon=1e-3)
    assert hi * hi - lo * lo > 0 and st["blended"].any() and (st["branch"] == R.BRANCH_ZERO).any()
    assert (st["branch"] == R.BRANCH_FULL).sum() > 20 * (st["branch"] == R.BRANCH_RAMP).sum()       # a step, not a ramp


def test_no_change_no_write(host_program, tmp_path):
    for W, H in SIZES:
        t, _, g = R.random_images(W, H, seed=11)
        t, _, _ = R.planted(t, t.copy(), g, seed=12)
        for radius in (1, 2, 3):
            out, st = check(host_program, tmp_path, t, t.copy(), g, **dict(R.DEFAULTS, Radius=radius))
            assert R.same(out, t) and not st["blended"].any()
