"""Motion-aware capture on the CPU: tests/motion_ref.py (the numpy binary32 restatement of the contract in include/idkpt.h, "motion-aware capture") against hand-computed
cases and against the per-pixel functions the device kernels call (idkengine_amd/csrc/motion_texel.hpp, reproject_texel.hpp) compiled for the host under ASan/UBSan as a
stand-alone program (tests/c_driver/motion_host.cpp), bit for bit: the motion record and the reprojection through a lookup record, on random inputs and on hand-made
adversarial ones.  With the lookup record equal to the geometry record the extended texel is the current one, bit for bit.  The host program's fetch aborts when it is
asked for a texel outside the image."""
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import motion_ref as MR  # noqa: E402
import reproject_ref as R  # noqa: E402
import test_reproject_ref as TR  # noqa: E402  (its analytic records and its tiny frame: inputs only)

F = np.float32
NAMES = ["idkptCaptureMotion", "idkptDownloadMotion", "idkptGetMotionDevicePtr"]
HIT = np.dtype([("T", "<f4"), ("BaryX", "<f4"), ("BaryY", "<f4"), ("TriangleId", "<u4"), ("MeshTransformId", "<u4"), ("Hit", "<u4")])


# ---- the feature exists
def test_the_library_declares_and_exports_the_motion_entry_points(tmp_path):
    from idkengine_amd import _lib, gputypes as T
    from idkengine_amd.pathtracer import PathTracer
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.idkptGetAbiVersion() == 13                   # (the entry points came without a new number: a host detects them by symbol)
    assert T.IDKPT_BUF_MOTION_PREV_POSITIONS == 13 and T.IDKPT_BUF_PREV_VERTEX_POSITIONS == 12
    assert L.idkptCaptureMotion(None, 0) == 2 and L.idkptDownloadMotion(None, 0, None, 0) == 2 and L.idkptGetMotionDevicePtr(None, 0, None, None) == 2
    for m in ("CaptureMotion", "DownloadMotion", "motion_device_ptr", "DownloadMotionPrevPositions"):
        assert callable(getattr(PathTracer, m))
    c = tmp_path / "e.c"
    c.write_text('#include <stdio.h>\n#include "idkpt.h"\nint main(void){printf("%d %d %d\\n", IDKPT_BUF_MOTION_PREV_POSITIONS, IDKPT_BUF_PREV_VERTEX_POSITIONS, IDKPT_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "e"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["13", "12", "13"]


# ---- the record by hand
def test_the_motion_record_by_hand():
    tris = np.uint32([[2, 0, 1, 9]])
    prev = F([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 4.0]])
    rows = F([[[1.0, 0.0, 0.0, 10.0], [0.0, 0.5, 0.0, 20.0], [0.0, 0.0, 2.0, 30.0]]])
    rec = MR.prev_records(F([0.25]), F([0.5]), [0], [0], tris, prev, rows)
    # b = (0.25, 0.5, 0.25) weighs vertices 2, 0, 1: l = 0.25 * (0, 0, 4) + 0.5 * (1, 0, 0) + 0.25 * (0, 2, 0) = (0.5, 0.5, 1)
    assert MR.same(rec[0], np.array([10.5, 20.25, 32.0, MR.asfloat(np.uint32([0]))[0]], F))
    rec = MR.prev_records(F([0.25]), F([0.5]), [0], [0], tris, prev, np.zeros((1, 3, 4), F))
    assert MR.same(rec[0, :3], F([0.0, 0.0, 0.0]))                           # a degenerate PrevModel of zeros: every point at the origin
    g = np.zeros((1, 2, 4), F); g[0, 0] = (0.1, 0.2, 0.3, MR.asfloat(np.uint32([0xFFFFFFFF]))[0]); g[0, 1] = (7.0, 8.0, 9.0, MR.asfloat(np.uint32([0]))[0])
    hits = np.zeros(2, HIT); hits["Hit"] = (0, 1); hits["BaryX"] = 0.25; hits["BaryY"] = 0.5
    img = MR.motion_image(g, hits, tris, prev, rows)
    assert MR.same(img[0, 0], g[0, 0]) and MR.same(img[0, 1], np.array([10.5, 20.25, 32.0, MR.asfloat(np.uint32([0]))[0]], F))   # a miss keeps the geometry record


# ---- the host build of the kernels' per-pixel functions
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/c_driver/motion_host.cpp + csrc/motion_texel.hpp + csrc/reproject_texel.hpp under ASan and UBSan, as a stand-alone program"""
    return MR.build_host_program(str(tmp_path_factory.mktemp("motion_host") / "motion_host"))


def nan_same(a, b):
    """bit for bit, except that a NaN equals a NaN (which NaN an operation of two NaNs returns is not part of the contract)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((MR.bits(a) == MR.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def random_mesh(rng, nv=40, nt=60, nx=5):
    prev = (rng.standard_normal((nv, 3)) * 3.0).astype(F)
    tris = np.zeros((nt, 4), np.uint32); tris[:, :3] = rng.integers(0, nv, (nt, 3)); tris[:, 3] = rng.integers(0, 7, nt)
    rows = rng.standard_normal((nx, 3, 4)).astype(F)
    return tris, prev, rows


def random_hits(rng, N, nt, nx, miss_share=0.25):
    h = np.zeros(N, HIT)
    bx = rng.random(N); by = rng.random(N) * (1.0 - bx)
    h["BaryX"] = bx; h["BaryY"] = by; h["T"] = rng.random(N) * 10.0
    h["TriangleId"] = rng.integers(0, nt, N); h["MeshTransformId"] = rng.integers(0, nx, N); h["Hit"] = rng.random(N) >= miss_share
    h["T"][h["Hit"] == 0] = R.FLT_MAX; h["TriangleId"][h["Hit"] == 0] = 0xFFFFFFFF
    return h


def records(exe, tmp, o, d, hits, tris, prev, rows):
    """the host build's two records against the restatements; returns the motion records"""
    g, m = MR.host_records(exe, str(tmp), o, d, hits, tris, prev, rows)
    want_g = R.pack(o, d, hits["T"], hits["MeshTransformId"], hits["Hit"])
    assert nan_same(g, want_g)                                               # the geometry record is idkptCaptureGeometry's
    want_m = MR.motion_image(want_g[None], hits, tris, prev, rows)[0]
    assert nan_same(m, want_m), int((MR.bits(m) != MR.bits(want_m)).any(axis=1).sum())
    return m


def test_host_records_equal_the_restatement_on_random_inputs(host_program, tmp_path):
    rng = np.random.default_rng(5)
    for N in (1, 257, 4000):
        tris, prev, rows = random_mesh(rng)
        hits = random_hits(rng, N, len(tris), len(rows))
        o = rng.standard_normal(3).astype(F); d = rng.standard_normal((N, 3)).astype(F)
        m = records(host_program, tmp_path, o, d, hits, tris, prev, rows)
        miss = hits["Hit"] == 0
        assert MR.same(m[miss, :3], d[miss]) and (MR.bits(m[miss, 3]) == 0xFFFFFFFF).all() and (MR.bits(m[~miss, 3]) == hits["MeshTransformId"][~miss]).all()
        assert np.isfinite(m[:, :3]).all()
    assert miss.any() and (~miss).any()


def test_host_records_equal_the_restatement_on_adversarial_inputs(host_program, tmp_path):
    rng = np.random.default_rng(6)
    tris, prev, rows = random_mesh(rng)
    model = rows.copy()                                                      # "Model": PrevModel == Model is the static instance
    eps = float(np.finfo(F).eps)
    # barycentrics 0, 1, and slightly outside the triangle on every side
    bary = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (-eps, 0.5), (0.5, -eps), (0.5 + eps, 0.5), (1.0 + 2 * eps, -eps), (-1e-3, -1e-3), (-0.0, 1.0)]
    hits = np.zeros(len(bary) * len(tris), HIT)
    hits["BaryX"] = np.tile(F([b[0] for b in bary]), len(tris)); hits["BaryY"] = np.tile(F([b[1] for b in bary]), len(tris))
    hits["TriangleId"] = np.repeat(np.arange(len(tris), dtype=np.uint32), len(bary)); hits["MeshTransformId"] = hits["TriangleId"] % len(rows); hits["Hit"] = 1; hits["T"] = 1.0
    o = F([0.0, 0.0, 0.0]); d = rng.standard_normal((len(hits), 3)).astype(F)
    m = records(host_program, tmp_path, o, d, hits, tris, prev, rows)
    t = tris[hits["TriangleId"]]
    for k, (corner, bxy) in enumerate([(1, (1.0, 0.0)), (2, (0.0, 1.0)), (3, (0.0, 0.0))]):   # a corner is its vertex (exactly where the other two terms are +-0)
        sel = (hits["BaryX"] == F(bxy[0])) & (hits["BaryY"] == F(bxy[1])) & (MR.bits(hits["BaryX"]) >> 31 == 0)
        q = prev[t[sel, corner - 1]]; Rw = rows[hits["MeshTransformId"][sel]]
        want = np.stack([((Rw[:, r, 0] * q[:, 0] + Rw[:, r, 1] * q[:, 1]) + Rw[:, r, 2] * q[:, 2]) + Rw[:, r, 3] for r in range(3)], -1)
        assert sel.any() and MR.same(m[sel, :3], want.astype(F)), corner
    # PrevModel == Model and previous positions == positions: the record is the world position of the hit point (here: of the same barycentric point) under Model
    assert MR.same(records(host_program, tmp_path, o, d, hits, tris, prev, model), m)
    # a degenerate PrevModel of zeros
    z = records(host_program, tmp_path, o, d, hits, tris, prev, np.zeros_like(rows))
    assert (z[:, :3] == 0.0).all() and (MR.bits(z[:, 3]) == hits["MeshTransformId"]).all()
    # NaN / Inf in a previous position or in PrevModel: the record carries it
    for bad in (np.nan, np.inf, -np.inf):
        p2 = prev.copy(); p2[tris[0, 0], 1] = bad
        r = records(host_program, tmp_path, o, d, hits, tris, p2, rows)
        touched = (tris[hits["TriangleId"], :3] == tris[0, 0]).any(axis=1)
        assert not np.isfinite(r[touched & (hits["BaryX"] == F(0.5)) & (hits["BaryY"] == F(0.5)), :3]).all(axis=1).any() and np.isfinite(r[~touched, :3]).all(), bad
        r2 = rows.copy(); r2[1, 2, 3] = bad
        r = records(host_program, tmp_path, o, d, hits, tris, prev, r2)
        sel = hits["MeshTransformId"] == 1
        assert not np.isfinite(r[sel, 2]).any() and np.isfinite(r[sel, :2]).all() and np.isfinite(r[~sel, :3]).all(), bad
    # ids outside the tables (never returned by the closest-hit core): the geometry record, and no read outside (ASan)
    wild = hits[:6].copy(); wild["TriangleId"][:2] = (len(tris), 0xFFFFFFFF); wild["MeshTransformId"][2:4] = (len(rows), 0x7FFFFFFF)
    t2 = tris.copy(); t2[wild["TriangleId"][4], 2] = len(prev); t2[wild["TriangleId"][5], 0] = 0xFFFFFFF0
    g, m = MR.host_records(host_program, str(tmp_path), o, d[:6], wild, t2, prev, rows)
    assert MR.same(g, m)


def check_texel(exe, tmp, cur, n, g, l, hg, hc, M, vp, moments=False, **s):
    st = {}
    if moments:
        want = MR.reproject_moments(cur, n, g, l, hg, hc, M, vp, stats=st, **s)
    else:
        want = MR.reproject(cur, n, g, l, hg, hc, M, vp, stats=st, **s)
    got = MR.host_texel(exe, str(tmp), cur, n, g, l, hg, hc, M, vp, moments=moments, **s)
    assert MR.same(got, want), int((MR.bits(got) != MR.bits(want)).any(axis=2).sum())
    return want, st


def moving_frames(W, H, rng, shift):
    """a history frame and a current frame of TR's wall and square under one camera; the square (id 1) moved by `shift` between them: returns what both reprojections need"""
    from idkengine_amd import scenes as S
    cam = S.Camera(W, H, position=(0.2, 0.1, 2.0), view_dir=(0.0, 0.0, -1.0), fovy_deg=80.0)
    hg = R.pack(*TR.analytic_records(cam, W, H))
    # the current frame: the square stands `shift` further; its records are the history's translated (same pixels, for the inputs' sake) and its previous positions the history's
    g = hg.copy(); sq = MR.bits(g[..., 3]) == 1
    g[sq, :3] = (g[sq, :3] + F(shift)).astype(F)
    l = g.copy(); l[sq, :3] = hg[sq, :3]
    cur = rng.random((H, W, 4)).astype(F); cur[..., 3] = 1.0
    hc = (rng.random((H, W, 4)) * 2.0).astype(F); hc[..., 3] = rng.integers(1, 60, (H, W)).astype(F)
    return cam, g, l, hg, hc, cur, sq


def test_host_texel_equals_the_restatement_and_follows_a_mover(host_program, tmp_path):
    W, H = 37, 23
    rng = np.random.default_rng(12)
    cam, g, l, hg, hc, cur, sq = moving_frames(W, H, rng, (0.0, 0.0, 0.3))    # towards the camera: ACROSS its surface (a surface that moves along itself finds other points of itself)
    M = (cam.view @ cam.proj).astype(F)
    assert sq.sum() >= 10 and (~sq).sum() >= 10                              # (the inputs hold a mover and a static rest)
    for n, s in ((1, {}), (3, dict(PositionTolerance=1e-3, MaxHistory=8.0))):
        plain, st0 = check_texel(host_program, tmp_path, cur, n, g, g, hg, hc, M, cam.position, **s)
        moved, st1 = check_texel(host_program, tmp_path, cur, n, g, l, hg, hc, M, cam.position, **s)
        assert not st0["history"][sq].any() and st0["position"][sq].any()    # the geometry record alone: the square moved by more than the tolerance, every pixel of it starts over
        assert st1["history"][sq].all()                                      # through the previous position every pixel of it finds itself
        assert MR.same(plain[~sq], moved[~sq])                               # (the static pixels' lookup record is their geometry record)
        mom = cur.copy(); mom[..., 2] = 0.0
        cnt, _ = check_texel(host_program, tmp_path, mom, n, g, l, hg, hc, M, cam.position, moments=True, **s)
        assert MR.same(cnt[..., 3], moved[..., 3]) and (cnt[..., 2] == 0.0).all()   # the moments' count is the temporal alpha
    # random lookup records anywhere near the scene: host and restatement agree whatever the record says
    wild = g.copy(); wild[..., :3] += (rng.standard_normal((H, W, 3)) * 0.05).astype(F)
    _, st = check_texel(host_program, tmp_path, cur, 2, g, wild, hg, hc, M, cam.position)
    assert st["history"].any() and st["position"].any()


def test_with_the_geometry_record_as_lookup_the_extended_texel_is_the_current_one(host_program, tmp_path):
    from idkengine_amd import scenes as S
    W, H = 37, 23
    rng = np.random.default_rng(13)
    prev = S.Camera(W, H, position=(0.2, 0.1, 2.0), view_dir=(0.0, 0.0, -1.0), fovy_deg=80.0)
    hg = R.pack(*TR.analytic_records(prev, W, H)); M = (prev.view @ prev.proj).astype(F)
    took = 0
    for mv in (dict(position=(0.25, 0.1, 2.0), view_dir=(0.05, 0.0, -1.0)), dict(position=(1.5, 0.4, 1.0), view_dir=(-0.6, 0.0, -1.0)), dict(position=(0.2, 0.1, -8.0), view_dir=(0.0, 0.0, 1.0))):
        g = R.pack(*TR.analytic_records(S.Camera(W, H, fovy_deg=80.0, **mv), W, H))
        cur = rng.random((H, W, 4)).astype(F); cur[..., 3] = 1.0
        hc = (rng.random((H, W, 4)) * 2.0).astype(F); hc[..., 3] = rng.integers(1, 60, (H, W)).astype(F)
        hc[3, 4, 1] = np.nan; hc[5, 6, 3] = np.inf
        for n, s in ((1, {}), (4, dict(PositionTolerance=0.5, MaxHistory=1.0))):
            st = {}
            want = R.reproject(cur, n, g, hg, hc, M, prev.position, stats=st, **s)          # the restatement of the current contract
            took += int(st["history"].sum())
            assert MR.same(MR.reproject(cur, n, g, g, hg, hc, M, prev.position, **s), want)
            assert MR.same(MR.host_texel(host_program, str(tmp_path), cur, n, g, None, hg, hc, M, prev.position, **s), want)     # reproject_texel(f, P, cur, g)
            assert MR.same(MR.host_texel(host_program, str(tmp_path), cur, n, g, g, hg, hc, M, prev.position, **s), want)        # reproject_texel(f, P, cur, g, g)
            for ext in (None, g):
                got = MR.host_texel(host_program, str(tmp_path), cur, n, g, ext, hg, hc, M, prev.position, moments=True, **s)
                assert MR.same(got[..., 3], want[..., 3]) and MR.same(got, MR.reproject_moments(cur, n, g, g, hg, hc, M, prev.position, **s))
    assert took > 0


def test_a_lookup_record_that_is_not_finite_takes_no_history(host_program, tmp_path):
    W = H = 4
    vp = (0.0, 0.0, 5000.0)
    Mw = TR.IDENT.copy(); Mw[15] = 0.0; Mw[11] = 1.0                         # a second matrix with clip.w = p'.z
    for M, z in ((TR.IDENT, -3.0), (Mw, 2.0)):
        cur, g, hg, hc = TR.tiny(seed=3)
        g[..., 2] = F(z); hg[..., 2] = F(z)
        base, st = check_texel(host_program, tmp_path, cur, 2, g, g, hg, hc, M, vp)
        assert st["history"].all()
        for bad in (np.nan, np.inf, -np.inf):
            for ch in (0, 1, 2):
                l = g.copy(); l[1, 1, ch] = bad
                out, st = check_texel(host_program, tmp_path, cur, 2, g, l, hg, hc, M, vp)
                assert not st["history"][1, 1] and MR.same(out[1, 1], np.append(cur[1, 1, :3], F(2.0)).astype(F)), (bad, ch)
                keep = np.ones((H, W), bool); keep[1, 1] = False
                assert MR.same(out[keep], base[keep])
