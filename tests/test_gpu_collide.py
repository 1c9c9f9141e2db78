"""idkptCollideSpheres / idkptCollideSpheresDevice (k_collide_spheres, csrc/kernels_collide.hpp): the engine's moving-sphere routine on the resident BVH.  Every comparison
is byte equality with tests/collide_ref.py, the numpy binary32 restatement of Intersections.SceneVsMovingSphereCollisionRoutine (NaNs by class where non-finite inputs are planted)."""
import copy
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import collide_ref as R  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def random_spheres(n, seed, extent=1.3, max_radius=0.3, max_move=0.5):
    """centres inside and around the box, radii 0 .. max_radius, displacements 0 .. max_move in a random direction"""
    rng = np.random.default_rng(seed)
    prev = rng.uniform(-extent, extent, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    dest = (prev + d * rng.uniform(0, max_move, (n, 1))).astype(F)
    return R.make_spheres(prev, rng.uniform(0, max_radius, n).astype(F), dest, rng.uniform(-1, 1, (n, 3)).astype(F))


@pytest.fixture(scope="module")
def cornell(native_builder):
    return S.cornell_scene(native_builder, "mixed", True)


@pytest.fixture(scope="module")
def cornell_pt(cornell):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(8, 8); pt.UploadScene(cornell)
    yield pt
    pt.Dispose()


def raw_call(pt, settings, spheres, out, count=None, fn="idkptCollideSpheres"):
    """the C entry point itself: returns its status"""
    return getattr(pt._L, fn)(pt._ctx, C.addressof(settings) if settings is not None else None, spheres.ctypes.data if spheres is not None else None,
                              len(spheres) if count is None else count, out.ctypes.data if out is not None else None)


@pytest.mark.parametrize("steps", [(1, 1), (3, 12), (1, 8), (20, 20)])
@pytest.mark.parametrize("response", [0, 1, 2])
@pytest.mark.parametrize("use_tlas", [0, 1])
def test_random_spheres_in_the_cornell_box(cornell, cornell_pt, use_tlas, response, steps):
    spheres = random_spheres(1000, 100 + steps[0])
    kw = dict(test_steps=steps[0], recursive_steps=steps[1], epsilon=0.001, response=response, use_tlas=bool(use_tlas))
    want, rep = R.collide(cornell, spheres, **kw)
    got = cornell_pt.CollideSpheres(spheres, **kw)
    assert got.tobytes() == want.tobytes(), int((got.view(np.uint32).reshape(1000, -1) != want.view(np.uint32).reshape(1000, -1)).any(axis=1).sum())
    assert (want["HitCount"] > 0).sum() >= 200 and (want["HitCount"] == 0).sum() >= 200 and int(want["HitCount"].max()) == steps[1]
    cornell_pt.synchronize()                                                     # (a raised overflow flag would fail here)


def directed_cornell():
    """name -> (sphere, settings, what the restatement's own report must show for the case to test anything)"""
    big = 0xFFFFFFFF
    return {
        # the floor (y = -1) is two triangles: its centre projects onto their shared diagonal, both are exactly as far away and the first one visited keeps the hit
        "diagonal": (R.make_spheres([(0.0, -0.5, 0.0)], 0.125, [(0.0, -0.9375, 0.0)]), dict(test_steps=1, recursive_steps=1, response=0),
                     lambda o, r: r["ties"][0] > 0 and o["HitCount"][0] == 1),
        # pushed diagonally into the edge where the floor meets the left wall: slides along one, then hits the other
        "corner": (R.make_spheres([(-0.6, -0.6, 0.1)], 0.25, [(-1.1, -1.1, 0.1)]), dict(test_steps=4, recursive_steps=8, response=1),
                   lambda o, r: o["HitCount"][0] >= 2),
        # the second of two steps puts the centre exactly on the floor: distance == 0 is rejected, the sphere passes through
        "on_triangle": (R.make_spheres([(0.25, -0.5, 0.25)], 0.125, [(0.25, -1.5, 0.25)]), dict(test_steps=2, recursive_steps=4, response=2),
                        lambda o, r: r["zero"][0] > 0),
        "far": (R.make_spheres([(50.0, 60.0, 70.0)], 0.25, [(51.0, 60.5, 69.0)]), dict(test_steps=3, recursive_steps=8, response=2),
                lambda o, r: o["HitCount"][0] == 0 and o["TriangleId"][0] == big and o["BlasInstanceId"][0] == big and r["visited"][0] == 0
                and o["Center"][0].tobytes() == (((np.array((50, 60, 70), F) + np.array((1, 0.5, -1), F) / F(3)) + np.array((1, 0.5, -1), F) / F(3)) + np.array((1, 0.5, -1), F) / F(3)).tobytes()
                and o["Center"][0].tobytes() != np.array((51, 60.5, 69), F).tobytes()),
        "radius_0": (R.make_spheres([(0.0, -0.5, 0.0)], 0.0, [(0.0, -1.5, 0.0)]), dict(test_steps=4, recursive_steps=4, response=1),
                     lambda o, r: r["visited"][0] > 0 and o["HitCount"][0] == 0),
        "nan_centre": (R.make_spheres([(np.nan, -0.5, 0.0)], 0.25, [(0.0, -1.5, 0.0)]), dict(test_steps=2, recursive_steps=4, response=1),
                       lambda o, r: r["visited"][0] == 0 and o["HitCount"][0] == 0 and np.isnan(o["Center"][0][0])),
        # corners at +-Inf: Box.Transformed turns them into NaN (Inf * 0), the box that enters a BLAS overlaps nothing (include/idkpt.h)
        "inf_radius": (R.make_spheres([(0.0, -0.5, 0.0)], np.inf, [(0.0, -0.75, 0.0)]), dict(test_steps=2, recursive_steps=4, response=1),
                       lambda o, r: o["HitCount"][0] == 0 and (o["Center"][0] == np.array((0, -0.75, 0), F)).all()),
    }


@pytest.mark.parametrize("use_tlas", [0, 1])
@pytest.mark.parametrize("name", sorted(directed_cornell()))
def test_directed_cases(cornell, cornell_pt, name, use_tlas):
    spheres, kw, shows = directed_cornell()[name]
    kw = dict(kw, epsilon=0.001, use_tlas=bool(use_tlas))
    want, rep = R.collide(cornell, spheres, **kw)
    assert shows(want, rep), (name, want, rep)                                    # the case is what its name says, on the restatement's own report
    got = cornell_pt.CollideSpheres(spheres, **kw)
    assert R.same_bits(got, want), (name, got, want)
    if name not in ("nan_centre", "inf_radius"):
        assert got.tobytes() == want.tobytes()


def test_a_radius_that_covers_the_scene_visits_every_leaf(native_builder):
    """one BLAS of 3 000 triangles, a sphere around all of it: every leaf is visited in every step and the walk uses the deepest stack the tree can ask for"""
    from idkengine_amd.pathtracer import PathTracer
    sc = S.soup_scene(3000, native_builder, seed=4)
    spheres = R.make_spheres([(0.5, 0.25, -0.5), (30.0, 0.0, 0.0)], [40.0, 45.0], [(0.75, 0.5, -0.25), (29.0, 0.0, 0.0)])
    pt = PathTracer(8, 8); pt.UploadScene(sc)
    for use_tlas in (False, True):
        for steps in ((1, 1), (2, 2)):                                           # (1, 1): exactly one walk, all 3 000 triangles; (2, 2): the pushed-out sphere walks again
            kw = dict(test_steps=steps[0], recursive_steps=steps[1], epsilon=0.001, response=2, use_tlas=use_tlas)
            want, rep = R.collide(sc, spheres, **kw)
            assert (rep["visited"] == 3000).all() if steps == (1, 1) else (rep["visited"] > 3000).any()
            assert (want["HitCount"] > 0).all()
            got = pt.CollideSpheres(spheres, **kw)
            assert got.tobytes() == want.tobytes()
            pt.synchronize()                                                     # the overflow flag is clear: a raised one turns into an error here
    pt.Dispose()


def test_results_do_not_depend_on_the_batch_size(cornell, cornell_pt):
    spheres = random_spheres(257, 7)
    kw = dict(test_steps=3, recursive_steps=6, epsilon=0.001, response=1, use_tlas=False)
    want, _ = R.collide(cornell, spheres, **kw)
    for n in (0, 1, 63, 64, 65, 257):
        got = cornell_pt.CollideSpheres(spheres[:n], **kw)
        assert len(got) == n and got.tobytes() == want[:n].tobytes(), n
    st = T.CollideSettings(3, 6, 0.001, 1, 0)
    assert raw_call(cornell_pt, st, None, None, count=0) == 0                     # count == 0 succeeds and touches nothing


def _host_state(pt, sc):
    """the scene as the device holds it now (nodes and TLAS as refitted / rebuilt there: tests/test_gpu_scene_updates.py holds those to the oracle)"""
    h = copy.copy(sc)
    h.blas_nodes = pt.DownloadBuffer(T.IDKPT_BUF_BLAS_NODES, T.GpuBlasNode, len(sc.blas_nodes))
    h.tlas_nodes = pt.DownloadBuffer(T.IDKPT_BUF_TLAS_NODES, T.GpuTlasNode, len(sc.tlas_nodes))
    return h


def test_queries_see_geometry_updates_and_leave_the_frame_alone(native_builder):
    from idkengine_amd.pathtracer import PathTracer
    tp = S.soup_triangles(1500, seed=14, extent=1.5, edge=0.4)
    p, i, nrm, tan = S.flat_shaded(tp)
    tp2 = S.soup_triangles(700, seed=15, extent=1.0, edge=0.4)
    p2, i2, n2, t2 = S.flat_shaded(tp2)
    sc = S.assemble([{"meshes": [S.MeshInput(p, i, S.make_material((0.8, 0.6, 0.5, 1.0)), nrm, tan)], "refittable": True},
                     {"meshes": [S.MeshInput(p2, i2, S.make_material((0.5, 0.7, 0.9, 1.0)), n2, t2)], "transform": S.translation((3.0, 0.0, 0.0))}], native_builder, sky_color=(0.7, 0.8, 1.0))
    w, h = 64, 48; cam = S.Camera(w, h, position=(0.0, 0.5, 9.0), fovy_deg=60.0)
    spheres = random_spheres(600, 21, extent=3.5, max_radius=0.4, max_move=0.8)
    for use_tlas in (False, True):
        kw = dict(test_steps=2, recursive_steps=4, epsilon=0.001, response=2, use_tlas=use_tlas)
        pt = PathTracer(w, h); pt.UploadScene(sc); pt.SetCamera(cam); pt.RayDepth = 3
        before = pt.CollideSpheres(spheres, **kw)
        assert before.tobytes() == R.collide(sc, spheres, **kw)[0].tobytes()
        # positions + refit
        nv = len(p)
        moved = sc.vertex_positions.copy(); moved[:nv] = (moved[:nv] + np.sin(moved[:nv, ::-1] * 1.7).astype(F) * F(0.2)).astype(F)
        pt.UpdateBuffer(T.IDKPT_BUF_VERTEX_POSITIONS, moved); pt.RefitBlas(0)
        h1 = _host_state(pt, sc); h1.vertex_positions = moved
        after1 = pt.CollideSpheres(spheres, **kw)
        assert after1.tobytes() == R.collide(h1, spheres, **kw)[0].tobytes() and after1.tobytes() != before.tobytes()
        # transforms + TLAS build on the device
        xf = sc.mesh_transforms.copy(); xf[1] = S.transform_from_matrix(S.rotation_y(40.0) @ S.translation((1.5, 0.4, 0.5)))[0]
        pt.UpdateBuffer(T.IDKPT_BUF_MESH_TRANSFORMS, xf); pt.BuildTlasOnDevice()
        h2 = _host_state(pt, h1); h2.vertex_positions = moved; h2.mesh_transforms = xf
        after2 = pt.CollideSpheres(spheres, **kw)
        assert after2.tobytes() == R.collide(h2, spheres, **kw)[0].tobytes() and after2.tobytes() != after1.tobytes()
        # a queued, unflushed sample in front of the query: the frame is what it is without the query
        pt.ResetAccumulation(); pt.Compute(); pt.Compute()
        again = pt.CollideSpheres(spheres, **kw)
        img = pt.Result.copy()
        assert again.tobytes() == after2.tobytes()
        pt.ResetAccumulation(); pt.Compute(); pt.Compute()
        assert pt.Result.tobytes() == img.tobytes()
        pt.Dispose()


def test_device_pointers_multi_device_and_the_python_mirror(cornell, cornell_pt):
    import torch
    from idkengine_amd.pathtracer import PathTracer, IdkPtError
    spheres = random_spheres(1001, 9)
    kw = dict(test_steps=3, recursive_steps=6, epsilon=0.001, response=2, use_tlas=True)
    st = T.CollideSettings(3, 6, 0.001, 2, 1)
    host = np.zeros(len(spheres), T.SphereCollision)
    assert raw_call(cornell_pt, st, spheres, host) == 0
    assert host.tobytes() == R.collide(cornell, spheres, **kw)[0].tobytes()
    assert cornell_pt.CollideSpheres(spheres, **kw).tobytes() == host.tobytes()    # the Python mirror returns the C call's bytes
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(np.frombuffer(spheres.tobytes(), np.uint8).copy()).to(dev)
    d_out = cornell_pt.CollideSpheres(d_in, **kw)
    assert d_out.is_cuda and d_out.cpu().numpy().tobytes() == host.tobytes()
    with pytest.raises(ValueError):
        cornell_pt.CollideSpheres(d_in[::2], **kw)                                # not contiguous
    with pytest.raises(ValueError):
        cornell_pt.CollideSpheres(d_in.cpu(), **kw)                               # not on the context's device
    grp = PathTracer(8, 8, devices=[0, 0]); grp.UploadScene(cornell)
    assert grp.CollideSpheres(spheres, **kw).tobytes() == host.tobytes()
    assert grp.CollideSpheres(spheres[:1], **kw).tobytes() == host[:1].tobytes()
    with pytest.raises(IdkPtError):
        grp.CollideSpheres(d_in, **kw)
    grp.Dispose()


def test_refusals_return_their_status_and_write_nothing(cornell, cornell_pt, native_builder):
    from idkengine_amd.pathtracer import PathTracer
    spheres = random_spheres(8, 3)
    canary = np.frombuffer(bytes([0xA5]) * (8 * 96), T.SphereCollision).copy()

    def refused(pt, st, s=spheres, count=None, null_out=False, status=2, fn="idkptCollideSpheres"):
        out = canary.copy()
        assert raw_call(pt, st, s, None if null_out else out, count=count, fn=fn) == status
        assert out.tobytes() == canary.tobytes()

    ok = (3, 6, 0.001, 1, 0)
    refused(cornell_pt, None)
    refused(cornell_pt, T.CollideSettings(*ok), s=None, count=8)
    refused(cornell_pt, T.CollideSettings(*ok), null_out=True)
    refused(cornell_pt, T.CollideSettings(*ok), count=1 << 31)
    for bad in ((3, 6, 0.001, 3, 0), (3, 6, 0.001, -1, 0), (0, 6, 0.001, 1, 0), (65, 6, 0.001, 1, 0), (3, -1, 0.001, 1, 0), (3, 65, 0.001, 1, 0),
                (3, 6, float("nan"), 1, 0), (3, 6, float("inf"), 1, 0)):
        refused(cornell_pt, T.CollideSettings(*bad))
        refused(cornell_pt, T.CollideSettings(*bad), fn="idkptCollideSpheresDevice")
    out = canary.copy()                                                          # the bounds themselves are accepted
    assert raw_call(cornell_pt, T.CollideSettings(64, 0, 0.0, 0, 0), spheres, out) == 0 and raw_call(cornell_pt, T.CollideSettings(1, 64, -0.5, 2, 1), spheres, out) == 0
    empty = PathTracer(8, 8)
    refused(empty, T.CollideSettings(*ok), status=3)                             # no scene
    empty.Dispose()
    no_tlas = copy.copy(cornell); no_tlas.tlas_nodes = np.zeros(0, T.GpuTlasNode)
    pt = PathTracer(8, 8); pt.UploadScene(no_tlas)
    refused(pt, T.CollideSettings(3, 6, 0.001, 1, 1), status=3)                  # UseTlas without TLAS nodes
    out = canary.copy()
    assert raw_call(pt, T.CollideSettings(*ok), spheres, out) == 0 and out.tobytes() == R.collide(cornell, spheres, 3, 6, 0.001, 1, False)[0].tobytes()
    pt.Dispose()
    grp = PathTracer(8, 8, devices=[0, 0]); grp.UploadScene(cornell)
    refused(grp, T.CollideSettings(3, 6, 0.001, 7, 0))
    refused(grp, T.CollideSettings(*ok), status=3, fn="idkptCollideSpheresDevice")
    grp.Dispose()
