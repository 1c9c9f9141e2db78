"""Temporal reprojection on the CPU: tests/reproject_ref.py (the numpy binary32 restatement of the contract in include/idkpt.h) against hand-computed cases and against the
per-pixel functions the device kernels call (idkengine_amd/csrc/reproject_texel.hpp) compiled for the host under ASan/UBSan as a stand-alone program
(tests/c_driver/reproject_host.cpp), bit for bit: the record packing and the reprojected pixel, on random records and cameras and on the edge cases of the contract.  The
host program's fetch aborts when it is asked for a texel outside the image, so every run also checks that no tap is fetched unchecked."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reproject_ref as R  # noqa: E402

F = np.float32
IDENT = np.eye(4, dtype=F).reshape(16)           # clip = (p.x, p.y, p.z, 1): u = (p.x * 0.5 + 0.5) * W - 0.5
NAMES = ["idkptCaptureGeometry", "idkptDownloadGeometry", "idkptGetGeometryDevicePtr", "idkptReproject", "idkptDownloadTemporal", "idkptGetTemporalDevicePtr",
         "idkptUseTemporalAsDenoised", "idkptSetDenoiseInput", "idkptGetDenoiseInput"]


# ---- the feature exists
def test_the_library_declares_and_exports_the_reprojection_entry_points():
    from idkengine_amd import _lib, gputypes as T
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.idkptGetAbiVersion() >= 12                  # (the entry points came without a new number: a host detects them by symbol)
    r = T.Reproject()
    assert C.sizeof(T.Reproject) == 84 and (r.PositionTolerance, r.MaxHistory) == (F(0.02), F(32.0)) and T.IDKPT_NO_HISTORY == R.NO_HISTORY == -2
    assert R.DEFAULTS == dict(PositionTolerance=0.02, MaxHistory=32.0)
    assert (T.IDKPT_DENOISE_INPUT_ACCUMULATED, T.IDKPT_DENOISE_INPUT_TEMPORAL) == (0, 1) and (T.IDKPT_RESULT_NOISY, T.IDKPT_RESULT_DENOISED) == (0, 1)
    # without a device the calls refuse a NULL context like every other entry point
    assert L.idkptCaptureGeometry(None, 0) == 2 and L.idkptReproject(None, 0, -2, None) == 2 and L.idkptDownloadTemporal(None, 0, None, 0) == 2
    assert L.idkptUseTemporalAsDenoised(None, 0) == 2 and L.idkptSetDenoiseInput(None, 1) == 2 and L.idkptGetDenoiseInput(None, None) == 2
    for m in ("CaptureGeometry", "Reproject", "DownloadGeometry", "DownloadTemporal", "UseTemporalAsDenoised", "SetDenoiseInput"):
        from idkengine_amd.pathtracer import PathTracer
        assert callable(getattr(PathTracer, m))


def test_struct_layout_matches_the_header(tmp_path):
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idkpt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(idkpt_reproject), '
                 'offsetof(idkpt_reproject, PrevProjView), offsetof(idkpt_reproject, PrevViewPos), offsetof(idkpt_reproject, PositionTolerance), offsetof(idkpt_reproject, MaxHistory), '
                 'IDKPT_NO_HISTORY, IDKPT_DENOISE_INPUT_ACCUMULATED, IDKPT_DENOISE_INPUT_TEMPORAL, IDKPT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    from idkengine_amd import gputypes as T
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    S = T.Reproject
    assert got[:8] == [C.sizeof(S), S.PrevProjView.offset, S.PrevViewPos.offset, S.PositionTolerance.offset, S.MaxHistory.offset, -2, 0, 1] and got[8] >= 12


# ---- hand-computed cases of the restatement
def ndc_for(u, W, exact=True):
    """the p.x whose previous pixel position under the identity matrix is exactly u (asserted in binary32)"""
    p = F((float(u) + 0.5) / W * 2.0 - 1.0)
    lo = hi = p
    for _ in range(16):                                   # (the estimate, then its neighbours: the expression rounds three times)
        for q in (lo, hi):
            if F(F(F(q * F(0.5)) + F(0.5)) * F(W)) - F(0.5) == F(u):
                return q
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
    if exact:
        raise AssertionError(("no binary32 p.x reaches", u, W))
    return p


def tiny(W=4, H=4, seed=0):
    """one surface (id 7) seen at the pixel centres by both frames under the identity matrix: every pixel finds itself, fx = fy = 0
    (exactly at sizes that are powers of two, to a rounding elsewhere)"""
    rng = np.random.default_rng(seed)
    g = np.zeros((H, W, 4), F)
    for y in range(H):
        for x in range(W):
            g[y, x] = (ndc_for(x, W, False), ndc_for(y, H, False), F(-3.0), R.asfloat(np.uint32([7]))[0])
    cur = rng.random((H, W, 4)).astype(F); cur[..., 3] = 1.0
    hc = rng.random((H, W, 4)).astype(F); hc[..., 3] = rng.integers(1, 20, (H, W)).astype(F)
    return cur, g, g.copy(), hc


def test_a_pixel_that_finds_itself_blends_by_the_sample_counts():
    cur, g, hg, hc = tiny()
    st = {}
    out = R.reproject(cur, 2, g, hg, hc, IDENT, (0, 0, 5), stats=st)
    assert st["history"].all() and not (st["clip_w"] | st["offscreen"] | st["id"] | st["colour"]).any()
    assert st["position"].any()                          # (the neighbours' taps, of weight 0, hold other points of the surface: rejected, and nothing changes)
    n = F(2.0)
    for (y, x) in [(0, 0), (3, 3), (1, 2)]:
        Hc = hc[y, x, 3]                                  # one tap of weight 1: h = hc * 1 / 1
        want = [F(F(F(hc[y, x, k] * Hc) + F(cur[y, x, k] * n)) / F(Hc + n)) for k in range(3)] + [F(Hc + n)]
        assert R.same(out[y, x], np.array(want, F))
    # the cap: a history of 19 samples counts as 4
    capped = R.reproject(cur, 1, g, hg, hc, IDENT, (0, 0, 5), MaxHistory=4.0)
    assert (capped[..., 3] <= 5.0).all() and (capped[..., 3] == np.minimum(hc[..., 3], 4.0) + 1.0).all()
    assert R.same(R.start(cur, 3)[..., :3], cur[..., :3]) and (R.start(cur, 3)[..., 3] == 3.0).all()


def test_the_bilinear_taps_and_their_order_by_hand():
    W = H = 4
    cur, g, hg, hc = tiny()
    g[1, 1, 0] = ndc_for(1.25, W); g[1, 1, 1] = ndc_for(2.5, H)      # x0 = 1, fx = 0.25; y0 = 2, fy = 0.5
    hg[...] = g[1, 1]                                                  # every history texel holds that surface point: all four taps valid
    out = R.reproject(cur, 1, g, hg, hc, IDENT, (0, 0, 5))
    fx, fy, one = F(0.25), F(0.5), F(1.0)
    w = [(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy]
    taps = [(2, 1), (2, 2), (3, 1), (3, 2)]                            # (y, x) of (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
    s = np.zeros(4, F); sw = F(0.0)
    for (ty, tx), wk in zip(taps, w):
        s = s + hc[ty, tx] * wk; sw = sw + wk
    h = s / sw; Hc = min(h[3], F(32.0)); n = F(1.0)
    assert R.same(out[1, 1], np.append((h[:3] * Hc + cur[1, 1, :3] * n) / (Hc + n), Hc + n).astype(F))


def test_the_record_by_hand():
    o = F([1.0, 2.0, 3.0]); d = F([[0.5, -0.25, 0.125], [0.0, 0.6, -0.8]])
    rec = R.pack(o, d, F([4.0, 3.4028235e38]), np.uint32([5, 0]), np.uint32([1, 0]))
    assert R.same(rec[0], np.array([3.0, 1.0, 3.5, R.asfloat(np.uint32([5]))[0]], F))
    assert R.same(rec[1, :3], d[1]) and R.bits(rec[1, 3:])[0] == 0xFFFFFFFF


# ---- the host build of the kernels' per-pixel functions
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/reproject_host.cpp + csrc/reproject_texel.hpp under ASan and UBSan, as a stand-alone program"""
    return R.build_host_program(str(tmp_path_factory.mktemp("reproject_host") / "reproject_host"))


def check(exe, tmp, cur, n, g, hg, hc, M, vp, **s):
    st = {}
    want = R.reproject(cur, n, g, hg, hc, M, vp, stats=st, **s)
    got = R.host_texel(exe, str(tmp), cur, n, g, hg, hc, M, vp, **s)
    assert R.same(got, want), int((R.bits(got) != R.bits(want)).any(axis=2).sum())
    return want, st


def analytic_records(cam, W, H):
    """records of a wall (id 0), a square in front of it (id 1) and the sky behind, seen by scenes.Camera `cam`: inputs only, nothing is held to them"""
    o, d = R.centre_rays(cam.inv_projection, cam.inv_view, W, H)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    T = np.full((H, W), 3.4028235e38, F); ids = np.zeros((H, W), np.uint32); hit = np.zeros((H, W), np.uint32)
    with np.errstate(all="ignore"):
        for z, half, k in ((-4.0, (3.0, 2.0), 0), (-2.0, (0.6, 0.6), 1)):  # the nearer one last: it wins
            t = (z - o64[2]) / d64[..., 2]
            p = o64 + d64 * t[..., None]
            ok = (t > 0) & (np.abs(p[..., 0]) < half[0]) & (np.abs(p[..., 1]) < half[1])
            T = np.where(ok, t.astype(F), T); ids = np.where(ok, np.uint32(k), ids); hit = np.where(ok, np.uint32(1), hit)
    return o, d, T, ids, hit


def test_host_build_equals_the_restatement_on_random_records_and_cameras(host_program, tmp_path):
    from idkengine_amd import scenes as S
    W, H = 37, 23
    rng = np.random.default_rng(11)
    seen = {k: 0 for k in ("clip_w", "offscreen", "id", "position", "history")}
    prev = S.Camera(W, H, position=(0.2, 0.1, 2.0), view_dir=(0.0, 0.0, -1.0), fovy_deg=80.0)
    hrec = analytic_records(prev, W, H)
    hg = R.pack(*hrec)
    assert R.same(R.host_pack(host_program, str(tmp_path), hrec[0], hrec[1].reshape(-1, 3), hrec[2].ravel(), hrec[3].ravel(), hrec[4].ravel()).reshape(H, W, 4), hg)
    assert (hrec[4] == 0).any() and (hrec[3] == 1).any() and ((hrec[4] == 1) & (hrec[3] == 0)).any()
    M = (prev.view @ prev.proj).astype(F)
    moves = [dict(position=(0.25, 0.1, 2.0), view_dir=(0.05, 0.0, -1.0)), dict(position=(0.2, 0.1, 2.0), view_dir=(0.3, -0.1, -1.0)), dict(position=(1.5, 0.4, 1.0), view_dir=(-0.6, 0.0, -1.0)),
             dict(position=(0.2, 0.1, -8.0), view_dir=(0.0, 0.0, 1.0)), dict(position=(0.2, 0.1, 2.0), view_dir=(0.0, 0.0, -1.0))]
    for i, mv in enumerate(moves):                                           # a small move, a rotation, a large move, a camera behind the wall looking back, no move at all
        cam = S.Camera(W, H, fovy_deg=80.0, **mv)
        rec = analytic_records(cam, W, H)
        g = R.pack(*rec)
        assert R.same(R.host_pack(host_program, str(tmp_path), rec[0], rec[1].reshape(-1, 3), rec[2].ravel(), rec[3].ravel(), rec[4].ravel()).reshape(H, W, 4), g)
        cur = rng.random((H, W, 4)).astype(F); cur[..., 3] = 1.0
        hc = (rng.random((H, W, 4)) * 2.0).astype(F); hc[..., 3] = rng.integers(1, 60, (H, W)).astype(F)
        for n, s in ((1, {}), (3, dict(PositionTolerance=1e-3, MaxHistory=8.0)), (1, dict(PositionTolerance=0.5, MaxHistory=1.0))):
            _, st = check(host_program, tmp_path, cur, n, g, hg, hc, M, prev.position, **s)
            for k in seen:
                seen[k] += int(st[k].sum())
        if i == 4:
            assert st["history"].mean() > 0.9
    assert all(v > 0 for v in seen.values()), seen                         # every rule decided some pixel somewhere


def test_the_restated_centre_rays_are_the_oracles(host_program, tmp_path):
    from idkengine_amd import scenes as S
    for W, H, kw in ((37, 23, dict(position=(0.3, -0.2, 3.4), view_dir=(0.2, 0.1, -1.0), fovy_deg=40.0)), (64, 64, dict()), (70, 37, dict(position=(1.0, 2.0, 3.0), view_dir=(-1.0, -0.5, 0.2)))):
        cam = S.Camera(W, H, **kw)
        o, d = R.oracle_centre_rays(host_program, str(tmp_path), cam.inv_projection, cam.inv_view, W, H)
        ro, rd = R.centre_rays(cam.inv_projection, cam.inv_view, W, H)
        assert R.same(o, ro) and R.same(d, rd)


def float_product(target):
    """(fx, fy), multiples of 2^-24 in (0, 1), whose binary32 product is exactly `target`"""
    for near in (0.2, 0.3, 0.13, 0.1):
        i0 = int(round(near * 2 ** 24))
        for i in range(i0 & ~1, i0 + 512, 2):             # (a step of j moves the product by several ulps of the target: most i have no j; both even, so that the
            j = int(round(float(target) * 2 ** 48 / i))   #  identity matrix on a 4 x 4 image reaches them: ndc_for)
            fx, fy = F(i * 2.0 ** -24), F(j * 2.0 ** -24)
            if j % 2 == 0 and F(fx * fy) == F(target):
                return fx, fy
    raise AssertionError(target)


def test_host_build_equals_the_restatement_on_the_edges_of_the_contract(host_program, tmp_path):
    W = H = 4
    vp = (0.0, 0.0, 5000.0)                                                # the tolerance is 0.02 * ~5000 = ~100: the neighbouring surface points pass, a point 150 away does not
    ID7 = R.asfloat(np.uint32([7]))[0]; ID8 = R.asfloat(np.uint32([8]))[0]

    def run(edit, n=2, M=IDENT, pixel=(1, 1), size=(4, 4), **s):
        cur, g, hg, hc = tiny(*size, seed=3)
        edit(cur, g, hg, hc)
        out, st = check(host_program, tmp_path, cur, n, g, hg, hc, M, vp, **s)
        return out[pixel], {k: bool(v[pixel]) for k, v in st.items()}, cur[pixel]

    def is_start(o, cur, n=2):
        return R.same(o, np.append(cur[:3], F(n)).astype(F))

    # clip.w <= 0: negative, zero, NaN
    Mw = IDENT.copy(); Mw[15] = 0.0; Mw[11] = 1.0                            # clip.w = p.z
    for z in (-3.0, 0.0, -0.0, np.nan):
        o, st, c = run(lambda cur, g, hg, hc: g.__setitem__((1, 1, 2), F(z)), M=Mw)
        assert st["clip_w"] and not st["history"] and is_start(o, c), z
    o, st, c = run(lambda cur, g, hg, hc: (g.__setitem__((Ellipsis, 2), F(2.0)), hg.__setitem__((Ellipsis, 2), F(2.0))), M=Mw)
    assert st["history"] and not st["clip_w"]                               # (and a positive one divides: u = p.x / 2 ...)
    # u exactly -1 (no history), one ulp inside (x0 = -1, the weight of tap x0 + 1 = 0 is below 0.01), exactly W (no history), W minus one ulp (x0 = W - 1, its weight is below 0.01)
    o, st, c = run(lambda cur, g, hg, hc: g.__setitem__((1, 1, 0), ndc_for(-1.0, W)))
    assert st["offscreen"] and is_start(o, c)
    def just_inside(cur, g, hg, hc):                                        # (an image one pixel wide: the only width at which binary32 reaches -1 + 2^-24)
        g[1, 0, 0] = ndc_for(np.nextafter(F(-1.0), F(0.0)), 1)
    o, st, c = run(just_inside, pixel=(1, 0), size=(1, 4))
    assert not st["offscreen"] and not st["history"] and is_start(o, c)    # x0 = -1, fx = 2^-24: the tap inside the image weighs 2^-24
    o, st, c = run(lambda cur, g, hg, hc: g.__setitem__((1, 1, 0), ndc_for(-0.25, W)))
    assert not st["offscreen"] and st["history"]                            # x0 = -1, fx = 0.75: tap x0 + 1 = 0 carries 0.75
    o, st, c = run(lambda cur, g, hg, hc: g.__setitem__((1, 1, 0), ndc_for(float(W), W)))
    assert st["offscreen"] and is_start(o, c)
    def below_w(cur, g, hg, hc):                                            # (five pixels wide: u + 0.5 stays in u's binade and 5 t reaches it)
        g[1, 1, 0] = ndc_for(np.nextafter(F(5.0), F(0.0)), 5)
    o, st, c = run(below_w, size=(5, 4))
    assert not st["offscreen"] and not st["history"] and is_start(o, c)    # inside the image, but the one tap inside weighs 2^-22
    for axis, val in ((1, ndc_for(-1.0, H)), (1, ndc_for(float(H), H))):
        o, st, c = run(lambda cur, g, hg, hc: g.__setitem__((1, 1, axis), val))
        assert st["offscreen"] and is_start(o, c)
    # NaN and Inf positions: the current pixel's (no history by the range test or the position test), a tap's (that tap is dropped)
    for bad in (np.nan, np.inf, -np.inf):
        for ch in (0, 1, 2):
            o, st, c = run(lambda cur, g, hg, hc: g.__setitem__((1, 1, ch), F(bad)))
            assert not st["history"] and is_start(o, c), (bad, ch)
            o, st, c = run(lambda cur, g, hg, hc: hg.__setitem__((1, 1, ch), F(bad)))
            assert st["position"] and not st["history"] and is_start(o, c), (bad, ch)
    # NaN and Inf history colour and history count, FLT_MAX is finite
    for bad in (np.nan, np.inf, -np.inf):
        for ch in (0, 2, 3):
            o, st, c = run(lambda cur, g, hg, hc: hc.__setitem__((1, 1, ch), F(bad)))
            assert st["colour"] and not st["history"] and is_start(o, c), (bad, ch)
    o, st, c = run(lambda cur, g, hg, hc: hc.__setitem__((1, 1, 0), R.FLT_MAX))
    assert st["history"] and not st["colour"]
    # a position just inside and just outside the tolerance: |p - q|^2 against (0.02 * 0.02) * |p - PrevViewPos|^2
    def moved(delta):
        def f(cur, g, hg, hc):
            hg[1, 1, 2] = g[1, 1, 2] + F(delta)
        return f
    o, st, c = run(moved(50.0))
    assert st["history"] and not st["position"]
    o, st, c = run(moved(150.0))
    assert st["position"] and is_start(o, c)
    # id mismatch on one, three and four taps (fx = fy = 0.5: every tap weighs 0.25)
    def quarter(mismatch):
        def f(cur, g, hg, hc):
            g[1, 1, 0] = ndc_for(1.5, W); g[1, 1, 1] = ndc_for(1.5, H)
            for (y, x) in [(1, 1), (1, 2), (2, 1), (2, 2)]:
                hg[y, x, :3] = g[1, 1, :3]
            for (y, x) in mismatch:
                hg[y, x, 3] = ID8
        return f
    o1, st, c = run(quarter([(1, 2)]))
    assert st["id"] and st["history"]
    o3, st, c = run(quarter([(1, 1), (1, 2), (2, 1)]))
    assert st["id"] and st["history"] and not R.same(o1, o3)
    o4, st, c = run(quarter([(1, 1), (1, 2), (2, 1), (2, 2)]))
    assert st["id"] and not st["history"] and is_start(o4, c)
    # sumW just below and just at 0.01: three taps mismatch, the fourth weighs fx * fy
    def lone_tap(fx, fy):
        def f(cur, g, hg, hc):
            g[1, 1, 0] = ndc_for(fx, W); g[1, 1, 1] = ndc_for(fy, H)
            hg[..., 3] = ID8; hg[1, 1] = g[1, 1]
        return f
    at = float_product(F(0.01)); below = float_product(np.nextafter(F(0.01), F(0.0)))
    o, st, c = run(lone_tap(*at))
    assert st["history"] and st["id"]
    o, st, c = run(lone_tap(*below))
    assert not st["history"] and is_start(o, c)
    # history count above MaxHistory, at it, below it; MaxHistory 1
    for count, cap in ((33.0, 32.0), (32.0, 32.0), (5.0, 32.0), (1000.0, 1.0)):
        o, st, c = run(lambda cur, g, hg, hc: hc.__setitem__((1, 1, 3), F(count)), MaxHistory=cap)
        assert st["history"] and o[3] == F(min(count, cap) + 2.0)
    # a miss reprojected by direction: the translation row is dropped, ids are 0xFFFFFFFF on both sides, no position test
    MISSF = R.asfloat(np.uint32([0xFFFFFFFF]))[0]
    Mt = IDENT.copy(); Mt[12] = 100.0; Mt[13] = -50.0; Mt[3] = 0.0; Mt[7] = 0.0; Mt[11] = -1.0; Mt[15] = 7.0      # clip.w = -d.z for a direction
    def sky(cur, g, hg, hc):
        g[1, 1] = (F(0.25), F(0.25), F(-1.0), MISSF)                        # u = (0.25 * 0.5 + 0.5) * 4 - 0.5 = 2
        hg[2, 2] = (F(9.0), F(9.0), F(9.0), MISSF)                          # any direction at all: ids alone decide
    o, st, c = run(sky, M=Mt)
    assert st["history"] and not (st["position"] or st["offscreen"]) and o[3] == tiny(seed=3)[3][2, 2, 3] + F(2.0)   # (the taps of weight 0 hold the surface: other ids)
    o, st, c = run(lambda cur, g, hg, hc: g.__setitem__((1, 1), (F(0.25), F(0.25), F(-1.0), MISSF)), M=Mt)
    assert st["id"] and is_start(o, c)                                     # sky now, a surface then
    # n = 1, and a large n
    for n in (1, 4096):
        o, st, c = run(lambda cur, g, hg, hc: None, n=n)
        assert st["history"] and o[3] == F(n) + tiny(seed=3)[3][1, 1, 3]
