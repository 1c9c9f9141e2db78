"""History reconstruction on the CPU: tests/reconstruct_ref.py (the numpy binary32 restatement of the contract in include/idkpt.h, "history reconstruction") against
hand-computed cases and against the per-pixel function the device kernel calls (idkengine_amd/csrc/reconstruct_texel.hpp) compiled for the host under ASan/UBSan as a
stand-alone program (tests/c_driver/reconstruct_host.cpp), bit for bit, on random images and on planted NaN, infinities, FLT_MAX, subnormals and zero and negative
counts.  The host program's fetch aborts when it is asked for a texel outside the image."""
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reconstruct_ref as R  # noqa: E402

F = np.float32
SIZES = [(1, 1), (5, 3), (16, 16), (17, 33), (37, 23)]                       # (W, H)
STRIDES = (1, 3, 8)                                                         # (8 * 3 = 24 texels: taps leave every one of these images on every side)


# ---- the feature exists
def test_the_library_declares_and_exports_the_reconstruction_entry_point(tmp_path):
    from idkengine_amd import _lib, gputypes as T
    from idkengine_amd.pathtracer import PathTracer
    import ctypes as C
    L = _lib.load()
    assert "idkptReconstructHistory" in _lib.SYMBOLS and hasattr(L, "idkptReconstructHistory")
    assert L.idkptGetAbiVersion() == 13                   # (the entry point came without a new number: a host detects it by symbol)
    assert L.idkptReconstructHistory(None, 0, None) == 2
    assert callable(getattr(PathTracer, "ReconstructHistory"))
    d = T.Reconstruct()
    assert (d.Radius, d.Stride, d.FillBelow, F(d.AlbedoSigma), F(d.NormalSigma)) == (2, 3, 4.0, F(0.2), F(0.5)) and C.sizeof(d) == 20
    assert all(F(getattr(d, k)) == F(v) for k, v in R.DEFAULTS.items()) and len(R.DEFAULTS) == len(T.Reconstruct._fields_)
    c = tmp_path / "e.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idkpt.h"\nint main(void){idkpt_reconstruct r = {2, 3, 4.0f, 0.2f, 0.5f};'
                 'int32_t (*fn)(idkpt_ctx*, int32_t, const idkpt_reconstruct*) = idkptReconstructHistory; (void)fn;'
                 'printf("%d %zu %zu %zu %zu %zu %d\\n", r.Radius, sizeof(r), offsetof(idkpt_reconstruct, Stride), offsetof(idkpt_reconstruct, FillBelow), offsetof(idkpt_reconstruct, AlbedoSigma), offsetof(idkpt_reconstruct, NormalSigma), IDKPT_ABI_VERSION);return 0;}\n')
    obj = tmp_path / "e.o"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(obj)])   # (declared: it compiles)
    c2 = tmp_path / "s.c"
    c2.write_text(c.read_text().replace("int32_t (*fn)(idkpt_ctx*, int32_t, const idkpt_reconstruct*) = idkptReconstructHistory; (void)fn;", ""))
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c2), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["2", "20", "4", "8", "12", "16", "13"]


# ---- by hand
def flat(W, H, count=20.0, rgb=(2.0, 4.0, 6.0), ident=5):
    """one surface with one colour, one count and constant guides: every weight is 1, every sum exact"""
    t = np.empty((H, W, 4), F); t[..., :3] = F(rgb); t[..., 3] = count
    g = np.zeros((H, W, 4), F); g[..., 3] = R.asfloat(np.uint32([ident]))[0]
    a = np.full((H, W, 4), 0.5, F); n = np.zeros((H, W, 4), F); n[..., 2] = 1.0
    return t, g, a, n


S1 = dict(Radius=1, Stride=1, FillBelow=4.0, AlbedoSigma=0.5, NormalSigma=0.5)


def test_one_short_pixel_in_a_flat_surface_capped_by_fill_below():
    t, g, a, n = flat(9, 9)
    t[4, 4] = (10.0, 0.0, 1.0, 1.0)
    st = {}
    out = R.reconstruct(t, g, a, n, stats=st, **S1)
    # eight taps of k = 1 * 20: S = 160, s / S = (2, 4, 6); b = min(160, 4 - 1) = 3, den = 4: ((10, 0, 1) * 1 + (2, 4, 6) * 3) / 4
    assert st["S"][4, 4] == 160.0 and st["taps"][4, 4] == 8 and st["written"].sum() == 1
    assert R.same(out[4, 4], F([4.0, 3.0, 4.75, 1.0]))
    keep = np.ones((9, 9), bool); keep[4, 4] = False
    assert R.same(out[keep], t[keep])
    # Stride 3, Radius 2: 24 taps at distance 3 and 6, those at distance 6 outside the 9 x 9 image: 8 are left
    out = R.reconstruct(t, g, a, n, stats=st, **dict(S1, Radius=2, Stride=3))
    assert st["taps"][4, 4] == 8 and R.same(out[4, 4], F([4.0, 3.0, 4.75, 1.0]))
    # a neighbour of another surface is no tap, whatever it holds, and is itself left alone
    t[4, 5, :3] = 100.0; g[4, 5, 3] = R.asfloat(np.uint32([6]))[0]
    out = R.reconstruct(t, g, a, n, stats=st, **S1)
    assert st["S"][4, 4] == 140.0 and st["taps"][4, 4] == 7 and R.same(out[4, 4], F([4.0, 3.0, 4.75, 1.0])) and R.same(out[4, 5], t[4, 5])


def test_one_tap_whose_weight_leaves_s_below_the_cap():
    t, g, a, n = flat(3, 3, count=4.0, rgb=(3.0, 6.0, 0.0))
    g[..., 3] = R.asfloat(np.arange(100, 109, dtype=np.uint32)).reshape(3, 3)      # every pixel its own surface ...
    g[1, 2, 3] = g[1, 1, 3]                                                        # ... but the centre and its right neighbour
    t[1, 1] = (9.0, 0.0, 3.0, 1.0)
    a[1, 2, 0] = 1.0          # dist2 = 0.25, invA = 1 / 0.25 = 4: w = 1 / ((1 + 1) * 1) = 0.5; k = 0.5 * 4 = 2 = S < 4 - 1
    st = {}
    out = R.reconstruct(t, g, a, n, stats=st, **S1)
    # b = 2, den = 3, s / S = (3, 6, 0): ((9, 0, 3) * 1 + (3, 6, 0) * 2) / 3
    assert st["S"][1, 1] == 2.0 and st["taps"][1, 1] == 1 and R.same(out[1, 1], F([5.0, 4.0, 1.0, 1.0])) and st["written"].sum() == 1
    # the donor's count is FillBelow exactly: it gives, and is not filled itself
    assert t[1, 2, 3] == S1["FillBelow"] and st["branch"][1, 2] == R.BRANCH_KEPT


def test_a_pixel_at_fill_below_a_miss_and_a_pixel_without_donors_keep_their_bits():
    t, g, a, n = flat(9, 9)
    t[4, 4] = (10.0, 0.0, 1.0, 4.0)                        # c = FillBelow: not below it
    st = {}
    assert R.same(R.reconstruct(t, g, a, n, stats=st, **S1), t) and (st["branch"] == R.BRANCH_KEPT).all()
    t[4, 4, 3] = np.nextafter(F(4.0), F(0.0))              # one ulp below: filled
    out = R.reconstruct(t, g, a, n, stats=st, **S1)
    assert st["written"][4, 4] and not R.same(out[4, 4, :3], t[4, 4, :3]) and R.bits(out[4, 4, 3]) == R.bits(t[4, 4, 3])
    t[4, 4, 3] = 1.0
    g[..., 3] = R.asfloat(np.uint32([0xFFFFFFFF]))[0]      # a miss among misses with long histories: never filled
    assert R.same(R.reconstruct(t, g, a, n, stats=st, **S1), t) and (st["branch"] == R.BRANCH_KEPT).all()
    g[..., 3] = R.asfloat(np.uint32([5]))[0]
    t[..., 3] = 1.0                                        # every pixel short: nobody gives, S = 0 everywhere
    assert R.same(R.reconstruct(t, g, a, n, stats=st, **S1), t) and (st["branch"] == R.BRANCH_NO_TAPS).all()
    t1, g1, a1, n1 = flat(1, 1, count=1.0)
    assert R.same(R.reconstruct(t1, g1, a1, n1, **R.DEFAULTS), t1)           # a 1 x 1 image: no tap inside


def test_negative_and_zero_counts_by_hand():
    t, g, a, n = flat(9, 9)
    t[4, 4] = (10.0, 0.0, 1.0, 0.0)                        # c = 0: b = min(160, 4) = 4, den = 4: the gathered colour alone
    out = R.reconstruct(t, g, a, n, **S1)
    assert R.same(out[4, 4], F([2.0, 4.0, 6.0, 0.0]))
    t[4, 4, 3] = -4.0                                      # c = -4: b = min(160, 8) = 8, den = 4: ((10, 0, 1) * -4 + (2, 4, 6) * 8) / 4
    out = R.reconstruct(t, g, a, n, **S1)
    assert R.same(out[4, 4], F([-6.0, 8.0, 11.0, -4.0]))
    # den = 0 is a division by zero: not finite, the pixel keeps its bits.  c = -156, FillBelow = 4: b = min(160, 160) = 160, den = 4; c = -160: b = 160, den = 0
    t[4, 4, 3] = -160.0
    st = {}
    out = R.reconstruct(t, g, a, n, stats=st, **S1)
    assert st["branch"][4, 4] == R.BRANCH_NOT_FINITE and R.same(out, t)


# ---- the host build of the kernel's per-pixel function
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/reconstruct_host.cpp + csrc/reconstruct_texel.hpp under ASan and UBSan, as a stand-alone program"""
    return R.build_host_program(str(tmp_path_factory.mktemp("reconstruct_host") / "reconstruct_host"))


def check(exe, tmp, t, g, a, n, **s):
    st = {}
    want = R.reconstruct(t, g, a, n, stats=st, **s)
    got, written = R.host_reconstruct(exe, str(tmp), t, g, a, n, **s)
    assert R.same(got, want), (s, int((R.bits(got) != R.bits(want)).any(axis=2).sum()))      # (a written pixel is finite, a kept one keeps its bits: no NaN is ever made)
    assert (written == st["written"]).all()
    assert R.same(want[~st["written"]], t[~st["written"]]) and R.same(want[..., 3], t[..., 3])
    return want, st


def test_host_equals_the_restatement_on_random_images(host_program, tmp_path):
    seen = set()
    for W, H in SIZES:
        t, g, a, n = R.random_images(W, H, seed=100 * W + H)
        for radius in (1, 2, 3):
            for stride in STRIDES:
                for fill in (4.0, 8.5):
                    out, st = check(host_program, tmp_path, t, g, a, n, **dict(R.DEFAULTS, Radius=radius, Stride=stride, FillBelow=fill))
                    seen |= set(np.unique(st["branch"]).tolist())
                    assert np.isfinite(out[st["written"]]).all()
    assert {R.BRANCH_KEPT, R.BRANCH_NO_TAPS, R.BRANCH_WRITTEN} <= seen


def test_the_random_case_fills_caps_and_starves():
    W, H = 37, 23
    t, g, a, n = R.random_images(W, H, seed=100 * W + H)
    st = {}
    R.reconstruct(t, g, a, n, stats=st, **R.DEFAULTS)
    cap = F(4.0) - t[..., 3]
    w = st["written"]
    assert w.sum() >= 0.1 * W * H and (st["branch"] == R.BRANCH_NO_TAPS).sum() >= 3 and (st["branch"] == R.BRANCH_KEPT).sum() >= 0.3 * W * H
    assert (st["S"][w] > cap[w]).any() and (st["S"][w] < cap[w]).any()                 # both sides of the fminf


def test_host_equals_the_restatement_on_planted_texels(host_program, tmp_path):
    seen = set()
    for W, H in SIZES:
        clean = R.random_images(W, H, seed=7 * W + H)
        t, g, a, n = R.planted(*clean, seed=W + H)
        for radius in (1, 2, 3):
            for stride in STRIDES:
                out, st = check(host_program, tmp_path, t, g, a, n, **dict(R.DEFAULTS, Radius=radius, Stride=stride))
                seen |= set(np.unique(st["branch"]).tolist())
                assert np.isfinite(out[st["written"]]).all() and np.isfinite(t[st["written"]]).all()
    assert R.BRANCH_WRITTEN in seen and R.BRANCH_NOT_FINITE in seen
    assert not np.isfinite(t).all() and not np.isfinite(a).all() and not np.isfinite(n).all() and (t[..., 3] <= 0).any()


def test_fill_below_under_every_count_is_a_no_op(host_program, tmp_path):
    t, g, a, n = R.random_images(37, 23, seed=11)
    out, st = check(host_program, tmp_path, t, g, a, n, **dict(R.DEFAULTS, FillBelow=0.5))
    assert R.same(out, t) and not st["written"].any()
