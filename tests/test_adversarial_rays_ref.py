"""CPU proof that the adversarial ray classes (tests/adversarial_rays.py) are what they claim, and that the checker — the oracle — is right on them where an independent answer
exists.  tests/test_gpu_adversarial_rays.py compares every walk with the oracle on these rays; a GPU test that passes on accidentally tame inputs is what this file prevents: every
floor below is a literal, so that an edit of the generator cannot empty a class unnoticed."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import adversarial_rays as A  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from test_metamorphic import brute_force  # noqa: E402

LATTICES = ("lattice", "lattice_refit", "lattice_inst", "lattice_same_space")


@pytest.fixture(scope="module")
def data(native_builder, oracle_mod):
    """per scene: the scene, its batch and the oracle's closest hits through the instance loop — computed once, never modified"""
    out = {}
    for name in A.SCENES:
        sc = A.make_scene(name, native_builder)
        rays, cls, kinds = A.make_rays(name, sc, lambda r, sc=sc: oracle_mod.trace_rays(sc, r))
        out[name] = (sc, rays, cls, kinds, oracle_mod.trace_rays(sc, rays))
    return out


def test_scenes_are_what_the_generator_says(data):
    parts, planted = A.lattice_parts()
    tp = np.concatenate(parts)
    assert 1400 <= len(tp) <= 1600
    assert (tp * 8 == np.round(tp * 8)).all()                                                    # every coordinate is k/8
    assert (tp[planted["dup_of_part0"]] == tp[planted["dup_src_part0"]]).all() and (tp[planted["dup_of_last"]] == tp[planted["dup_src_last"]]).all()
    z = tp[planted["zero_area"]]; assert (np.cross(z[:, 1] - z[:, 0], z[:, 2] - z[:, 0]) == 0).all()
    s = tp[planted["slanted"]]; assert ((np.cross(s[:, 1] - s[:, 0], s[:, 2] - s[:, 0]) != 0).sum(1) >= 2).all()
    # PreSplit made fragments in exactly one of the two single-BLAS builds
    assert len(data["lattice"][0].blas_triangles) > len(tp) and len(data["lattice_refit"][0].blas_triangles) == len(tp)
    sc = data["lattice_inst"][0]
    assert len(sc.blas_descs) == 12 and len(sc.blas_instances) == 13
    assert sc.blas_instances["BlasId"][3] == sc.blas_instances["BlasId"][4] and sc.mesh_transforms[3].tobytes() == sc.mesh_transforms[4].tobytes()
    for i in A.EXACT_INSTANCES:                                                                  # exact matrices: 0, +-1 and dyadic translations, both ways
        for k in ("Model", "InvModel"):
            m = sc.mesh_transforms[i][k]
            assert np.isin(np.abs(m[:, :3]), (0.0, 1.0)).all() and (m[:, 3] * 8 == np.round(m[:, 3] * 8)).all(), (i, k)
    assert not np.isin(np.abs(sc.mesh_transforms[5]["Model"][:, :3]), (0.0, 1.0)).all()         # ... and one general rotation
    sc = data["lattice_same_space"][0]
    assert len(sc.blas_instances) == 12 and all(t.tobytes() == sc.mesh_transforms[0].tobytes() for t in sc.mesh_transforms)


def test_the_numpy_restatements_are_the_oracles_expressions(oracle_mod, data):
    """ray_triangle_f32 / box_slabs_f32 (numpy binary32) against ref_ray_triangle / ref_ray_box on adversarial rays x lattice triangles / nodes: same decision, same T bits"""
    L = oracle_mod.lib()
    sc, rays, cls, _, _ = data["lattice"]
    rng = np.random.default_rng(2)
    ri = np.concatenate([rng.choice(np.nonzero(cls == A.CID[c])[0], 12, replace=False) for c in ("axis", "on_plane", "tiny", "edge", "vertex", "on_surface")])
    ti = rng.choice(len(sc.blas_triangles), 40, replace=False)
    t = sc.blas_triangles[ti]
    p = [np.ascontiguousarray(sc.vertex_positions[t[k]], np.float32) for k in ("X", "Y", "Z")]
    ok, tt = A.ray_triangle_f32(rays["Origin"][ri], rays["Direction"][ri], *p)
    bary = (C.c_float * 3)(); tv = C.c_float()
    for a, r in enumerate(rays[ri]):
        o = np.ascontiguousarray(r["Origin"]); d = np.ascontiguousarray(r["Direction"])
        for b in range(len(ti)):
            h = L.ref_ray_triangle(o.ctypes.data, d.ctypes.data, p[0][b].ctypes.data, p[1][b].ctypes.data, p[2][b].ctypes.data, bary, C.byref(tv))
            assert bool(h) == bool(ok[a, b])
            if h:
                assert np.float32(tv.value).tobytes() == tt[a, b].tobytes()
    nodes = sc.blas_nodes[1:][rng.choice(len(sc.blas_nodes) - 1, 60, replace=False)]
    lo, hi = A.box_slabs_f32(rays["Origin"][ri], rays["Direction"][ri], nodes["Min"], nodes["Max"])
    with np.errstate(all="ignore"):
        t1 = np.fmax(np.fmax(np.fmin(lo, hi)[..., 0], np.fmin(lo, hi)[..., 1]), np.fmax(np.fmin(lo, hi)[..., 2], np.float32(0)))      # fmin / fmax ignore a NaN operand (ref_math.h:45-49)
        t2 = np.fmin(np.fmin(np.fmax(lo, hi)[..., 0], np.fmax(lo, hi)[..., 1]), np.fmax(lo, hi)[..., 2])
    t1v = C.c_float(); nan_seen = 0
    for a, r in enumerate(rays[ri]):
        o = np.ascontiguousarray(r["Origin"]); d = np.ascontiguousarray(r["Direction"])
        for b, nd in enumerate(nodes):
            mn = np.ascontiguousarray(nd["Min"]); mx = np.ascontiguousarray(nd["Max"])
            h = L.ref_ray_box(o.ctypes.data, d.ctypes.data, mn.ctypes.data, mx.ctypes.data, C.byref(t1v))
            assert bool(h) == bool(t1[a, b] <= t2[a, b]), (a, b)
            nan_seen += int(np.isnan(lo[a, b]).any() or np.isnan(hi[a, b]).any())
    assert nan_seen > 0


@pytest.mark.parametrize("name", A.SCENES)
def test_every_class_is_what_it_claims(data, name):
    sc, rays, cls, kinds, hits = data[name]
    o, d = rays["Origin"], rays["Direction"]
    assert np.isfinite(o).all() and np.isfinite(d).all() and (np.abs(d).max(1) > 0).all() and not np.isnan(rays["MaxDist"]).any() and (rays["MaxDist"] >= 0).all()
    sel = lambda c: cls == A.CID[c]      # noqa: E731
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / d
    # axis: +-e_i, both signs of zero
    da = d[sel("axis")]
    assert len(da) >= 1400 and ((da == 0).sum(1) == 2).all() and (np.abs(da).max(1) == 1).all()
    assert (np.signbit(da) & (da == 0)).sum() >= 200 and (~np.signbit(da) & (da == 0)).sum() >= 200
    # planar: exactly one zero, unit length
    dp = d[sel("planar")]
    assert len(dp) >= 1400 and ((dp == 0).sum(1) == 1).all() and np.allclose(np.linalg.norm(dp.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # on_plane: the 0 * inf rays
    nan = A.nan_slab_mask(sc, rays[sel("on_plane")])
    assert nan.sum() >= 200, nan.sum()
    # tiny: non-finite 1/dir with non-zero dir; a finite 1/dir whose slab product overflows
    it, dt = inv[sel("tiny")], d[sel("tiny")]
    assert (np.isinf(it) & (dt != 0)).any(1).sum() >= 200
    a, b = A.box_slabs_f32(o[sel("tiny")], dt, sc.blas_nodes["Min"][1:2], sc.blas_nodes["Max"][1:2])
    assert ((np.isinf(a[:, 0]) | np.isinf(b[:, 0])) & np.isfinite(it)).any(1).sum() >= 200
    assert (np.isfinite(it).all(1) & (np.abs(it).max(1) > 1e29)).sum() >= 200
    # range: every kind on at least 100 rays that hit without the limit
    m = sel("range")
    assert (rays["MaxDist"][m][kinds[m] == 3] == 0).all() and np.isposinf(rays["MaxDist"][m][kinds[m] == 5]).all()
    for k in range(6):
        assert (kinds[m] == k).sum() >= 100, (A.RANGE_KINDS[k], (kinds[m] == k).sum())
    assert (hits["Hit"][m][np.isin(kinds[m], (0, 1, 3))] == 0).all()                             # `t < T`: at T, below it and at 0 nothing is hit
    assert (hits["Hit"][m][np.isin(kinds[m], (4, 5))] != 0).all()
    assert (hits["Hit"][m][kinds[m] == 2] != 0).mean() > 0.98                                    # one float above the hit: found (a walk may cull the leaf's box at that T)
    if name in LATTICES:
        # ties: two or more candidates accepted at the bits of the closest T — and the oracle's walk reports that T (it reached them)
        for c in ("edge", "vertex", "duplicate"):
            r = rays[sel(c)]; h = hits[sel(c)]
            n = A.closest_ties(sc, r)
            assert (n >= 2).sum() >= 200, (c, (n >= 2).sum())
            reached = (n >= 2) & (h["Hit"] != 0)
            assert reached.sum() >= 200, (c, reached.sum())
        n = A.closest_ties(sc, rays[sel("on_surface")]); h = hits[sel("on_surface")]
        assert ((h["Hit"] != 0) & (h["T"] == 0)).sum() >= 200                                    # t == 0 is accepted
    if name == "lattice_inst":
        # the doubled instance: hits on instance 3 / 4 are reported for the lower one
        h = hits[sel("duplicate")]
        assert ((h["Hit"] != 0) & (h["MeshTransformId"] == 3)).sum() >= 200 and (h["MeshTransformId"][h["Hit"] != 0] != 4).all()


@pytest.mark.parametrize("name", A.SCENES)
def test_oracle_is_self_consistent_on_these_rays(oracle_mod, data, name):
    """Any hit and closest hit agree on hit-or-miss, in both modes.  TLAS walk and instance loop agree on hit-or-miss and on T for rays without ties — and without a NaN slab: the
    loop tests a BLAS root box that the TLAS walk never tests (BVHIntersect.glsl:32-39), so a ray lying in a root box's plane can be dropped by one and found by the other; and
    with MaxDist more than an ulp away from T: the loop culls with `<`, the TLAS walk's leaves with `<=`."""
    sc, rays, cls, kinds, loop = data[name]
    tlas = oracle_mod.trace_rays(sc, rays, use_tlas=True)
    nan = A.nan_slab_mask(sc, rays)
    for use_tlas, closest in ((False, loop), (True, tlas)):
        a = oracle_mod.trace_rays(sc, rays, any_hit=True, use_tlas=use_tlas)
        assert ((a["Hit"] != 0) == (closest["Hit"] != 0)).all()
        ok = (a["Hit"] != 0) & ~nan            # (with a NaN slab which boxes a walk enters depends on its order: the closest-hit walk can lose a hit the any-hit walk finds)
        assert (a["T"][ok] >= closest["T"][ok]).all()
    plain = ~nan & (A.closest_ties(sc, rays, by_value=True) <= 1) & ~np.isin(kinds, (0, 1, 2))
    assert plain.sum() > 2000
    assert ((loop["Hit"] != 0) == (tlas["Hit"] != 0))[plain].all()
    assert (loop["T"].view(np.uint32) == tlas["T"].view(np.uint32))[plain].all()


@pytest.mark.parametrize("name,cname", [("soup", "axis"), ("soup", "planar"), ("lattice", "axis"), ("lattice", "planar")])
def test_zero_components_lose_no_hit_against_the_float64_brute_force(data, name, cname):
    """A zero direction component by itself (-inf / +inf slabs, no NaN) loses no hit: on ROBUST rays the oracle reports the triangle the float64 brute force
    (tests/c_driver/brute_force.c, no BVH) reports, and a float64 miss is an oracle miss.  Robust: (a) no origin coordinate along a zero axis equals a node bound of the scene's
    trees on that axis; (b) the float64 hit has every barycentric >= 1e-3, |dot(d, n)| >= 1e-3 |n| and t >= 1e-3 of the scene's extent; (c) no other triangle within 1e-3
    relative of t; (d) MaxDist not within 1e-3 relative of t.  1e-3 is about 1.6e4 binary32 ulps: a margin, not a measurement.  At least 90 % of the float64-hitting rays of the
    class must be robust (origins are drawn off the dyadic grid / rays are sent through triangle interiors for that)."""
    sc, rays, cls, _, hits = data[name]
    m = cls == A.CID[cname]
    r, h = rays[m], hits[m]
    tris, owner = A.world_triangles(sc)
    # PreSplit stores a triangle once per fragment: the copies are one triangle (the same three vertex ids), not "another triangle within 1e-3 of t"
    vid = lambda ids: np.stack([sc.blas_triangles[k][ids] for k in ("X", "Y", "Z")], 1)      # noqa: E731
    _, first = np.unique(np.c_[owner[:, 0], vid(owner[:, 1])], axis=0, return_index=True)
    tris, owner = tris[np.sort(first)], owner[np.sort(first)]
    o64, d64 = r["Origin"].astype(np.float64), r["Direction"].astype(np.float64)
    bt, bi, bt2 = brute_force(tris, o64, d64)
    f64hit = np.isfinite(bt) & (bi >= 0)
    assert f64hit.sum() >= 500, f64hit.sum()
    # (a)
    nodes = np.concatenate([sc.blas_nodes["Min"], sc.blas_nodes["Max"]] + ([sc.tlas_nodes["Min"], sc.tlas_nodes["Max"]] if len(sc.tlas_nodes) else []))
    on_bound = np.zeros(len(r), bool)
    for ax in range(3):
        on_bound |= (r["Direction"][:, ax] == 0) & np.isin(r["Origin"][:, ax], nodes[:, ax])
    # (b)
    t = tris[np.where(f64hit, bi, 0)]
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]; n = np.cross(e1, e2)
    P = o64 + d64 * np.where(f64hit, bt, 0.0)[:, None]
    den = (n * n).sum(1); den[den == 0] = 1.0
    b1 = (np.cross(P - t[:, 0], e2) * n).sum(1) / den; b2 = (np.cross(e1, P - t[:, 0]) * n).sum(1) / den
    extent = float(np.ptp(tris.reshape(-1, 3), 0).max())
    nl = np.linalg.norm(n, axis=1); nl[nl == 0] = 1.0
    b_ok = (np.minimum(np.minimum(b1, b2), 1.0 - b1 - b2) >= 1e-3) & (np.abs((d64 * n).sum(1)) >= 1e-3 * nl * np.linalg.norm(d64, axis=1)) & (bt >= 1e-3 * extent)
    # (c), (d)
    with np.errstate(invalid="ignore"):
        c_ok = ~(np.abs(bt2 - bt) <= 1e-3 * np.abs(bt))
    d_ok = ~(np.abs(r["MaxDist"].astype(np.float64) - bt) <= 1e-3 * np.abs(bt))
    robust = f64hit & ~on_bound & b_ok & c_ok & d_ok
    share = robust.sum() / f64hit.sum()
    print(f"{name}/{cname}: {f64hit.sum()} float64 hits, {robust.sum()} robust ({share:.3f})")
    assert share >= 0.9, share
    assert (h["Hit"][robust] != 0).all()
    assert (vid(h["TriangleId"][robust]) == vid(owner[bi[robust], 1])).all()
    miss = ~f64hit & ~on_bound
    assert (h["Hit"][miss] == 0).all()


def test_the_axis_aligned_rays_case_has_huge_but_finite_inverse_directions():
    """The `axis_aligned_rays` case of test_gpu_packet.py / test_gpu_wide.py (Camera fovy_deg = 1e-4 at 64 x 64): GetWorldSpaceDirection (pt_device.hpp) in binary32 for every
    pixel and the extreme jitters — the x / y components are around 1e-8, some 30 orders of magnitude above the 2.9e-39 below which binary32 1/x overflows.  1/dir is finite for
    every ray but one whose x + jitter is the frame's centre to the last bit: the case covers huge 1/dir, not non-finite ones."""
    w = h = 64
    cam = S.Camera(w, h, position=(0.0, 0.0, 3.4), fovy_deg=1e-4)
    ip, iv = cam.inv_projection.astype(np.float32), cam.inv_view.astype(np.float32)
    f = np.float32
    finite = 0; total = 0; smallest = np.inf
    for j in (f(0.0), f(2.0 ** -24), f(0.5), f(1.0 - 2.0 ** -24)):
        xs, ys = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        nx = (xs + j) / f(w) * f(2) - f(1); ny = (ys + j) / f(h) * f(2) - f(1)
        rx = ip[0] * nx + ip[4] * ny; ry = ip[1] * nx + ip[5] * ny
        v = np.stack([((iv[k] * rx + iv[4 + k] * ry) + iv[8 + k] * f(-1)) + iv[12 + k] * f(0) for k in range(3)], -1)
        d = v * (f(1) / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]))[..., None]
        with np.errstate(all="ignore"):
            inv = f(1) / d
        ok = np.isfinite(inv).all(-1)
        assert (ok | (nx == 0) | (ny == 0)).all()                      # non-finite only where a pixel's sample is the centre of the frame exactly
        finite += ok.sum(); total += ok.size
        nz = np.abs(d[..., :2][d[..., :2] != 0]); smallest = min(smallest, float(nz.min()))
    assert finite >= total - 4 * (w + h)
    assert smallest > 1e-15 and np.abs(inv[np.isfinite(inv)]).max() > 1e6


def test_the_stale_root_box_case_decides_between_strict_and_lenient_root_tests(native_builder, oracle_mod):
    """A.stale_root_scene: for the rays that come straight down, instance 1's root box is met at t1 == T of the hit on instance 0, bit for bit, instance 1 holds an accepted
    triangle at a smaller t, and the oracle — the loop, with its strict root test — still reports instance 0's hit."""
    sc = A.stale_root_scene(native_builder); rays = A.stale_root_rays()
    h = oracle_mod.trace_rays(sc, rays)
    down = (rays["Direction"][:, 2] == -1) & (rays["Direction"][:, 0] == 0) & (rays["MaxDist"] > 1)
    assert down.sum() >= 64
    assert (h["Hit"][down] != 0).all() and (h["MeshTransformId"][down] == 0).all() and (h["T"][down] == np.float32(0.75)).all()
    root = sc.blas_nodes[sc.blas_descs[1]["NodeOffset"] + 1]
    assert root["Max"][2] == np.float32(0.25)
    lo, hi = A.box_slabs_f32(rays["Origin"][down], rays["Direction"][down], root["Min"][None], root["Max"][None])
    with np.errstate(all="ignore"):
        t1 = np.fmax(np.fmax(np.fmin(lo, hi)[..., 0], np.fmin(lo, hi)[..., 1]), np.fmax(np.fmin(lo, hi)[..., 2], np.float32(0)))[:, 0]
    assert (t1.view(np.uint32) == h["T"][down].view(np.uint32)).all()
    d = sc.blas_descs[1]; t = sc.blas_triangles[d["TriangleOffset"]: d["TriangleOffset"] + d["TriangleCount"]]
    ok, tt = A.ray_triangle_f32(rays["Origin"][down], rays["Direction"][down], sc.vertex_positions[t["X"]], sc.vertex_positions[t["Y"]], sc.vertex_positions[t["Z"]])
    assert (np.where(ok, tt, np.inf).min(1) == np.float32(0.5)).all()                          # what a lenient root test would have found
    assert (h["Hit"][rays["MaxDist"] == np.float32(0.75)] == 0).all()                          # MaxDist == T of instance 0's hit: nothing (`t < T`), and no root box entered
    assert (oracle_mod.trace_rays(sc, rays, use_tlas=True)["T"][down] == np.float32(0.5)).all()   # (the TLAS walk tests no root box and finds the moved sheet: the modes differ here, legitimately)
