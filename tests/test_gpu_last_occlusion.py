"""The deferred last bounce traced hit-or-miss (developer option last_occlusion, csrc/kernels_trace.hpp k_trace2 OCCL): where k_shade_last<false> is the only reader of the
last bounce's hit records — no emission, no light hits — the launch stops every ray at its first accepted triangle, and the closest hits are traced when somebody asks for
the continuation (finish_deferred).  Nothing a host can read may depend on it: every comparison here is option 1 against option 0 on the same sequence of calls, bit for
bit (Result, idkptDownloadRays, idkptDownloadAliveQueue, alive_counts, rays_traced), the basic cases against the oracle as well; stats()["last_occlusion_launches"] says
which launch ran."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import configs  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import bits  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
# the tests' frames are tiny: the fused launch and the split kernel would take the bounce of a sparse view from the second batch on (want_fused / want_split), and neither has the flavour
ELIGIBLE = {"fused": 0, "split": 0}


@pytest.fixture(scope="module")
def soup(native_builder):
    return S.soup_scene(3000, native_builder, seed=7, extent=2.0, refittable=True)


def _cam(view, w=W, h=H):
    if view == "outside":
        return S.Camera(w, h, position=(0.0, 0.5, 9.0), fovy_deg=60.0)
    return S.Camera(w, h, position=(0.0, 0.0, 0.0), view_dir=(0.2, 0.1, -1.0))


def _pt(sc, cam, occl, w=W, h=H, batch=1, opts=None, **ov):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h, settings=configs.apply_settings(T.Settings.default(), ov))
    for k, v in (opts or {}).items():
        pt.set_option(k, v)
    pt.set_option("last_occlusion", occl)
    pt.UploadScene(sc); pt.SetCamera(cam); pt.set_max_batch(batch)
    return pt


def _snap(pt, state=True):
    """what a host can read, in the order frame -> statistics -> (on demand) ray state and queue"""
    out = {"image": bits(pt.Result).tobytes()}
    st = pt.stats()
    out["alive_counts"] = tuple(st["alive_counts"]); out["rays_traced"] = st["rays_traced"]
    if state:
        out["rays"] = pt.rays().tobytes(); out["queue"] = pt.alive_queue().tobytes()
        out["image_after"] = bits(pt.Result).tobytes()
        st = pt.stats(); out["alive_counts_after"] = tuple(st["alive_counts"]); out["rays_traced_after"] = st["rays_traced"]
    return out


def _both(run):
    """run(occl) -> (list of snapshots, hit-or-miss launches); the snapshots of option 1 must be option 0's"""
    want, n0 = run(0)
    got, n1 = run(1)
    assert n0 == 0
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        for k in a:
            assert a[k] == b[k], (i, k)
    return want, n1


@pytest.mark.parametrize("view", ["outside", "inside"])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("batch", [1, 3, 9])
def test_frames_state_and_counts_do_not_depend_on_it(soup, oracle_mod, view, depth, batch):
    """batch 9 is pixel-major (the first bounce traced from k_shade_first's list, hits per ray id, where it is the last bounce: depth 2); depth 3: the last bounce is
    j = 2 and reads k_shade's records"""
    cam = _cam(view)
    opts = dict(ELIGIBLE, bounce_pixel_major=2)

    def run(occl):
        pt = _pt(soup, cam, occl, batch=batch, opts=opts, RayDepth=depth)
        snaps = []
        for _ in range(2):
            for _ in range(batch):
                pt.Compute()
            snaps.append(_snap(pt))
        n = pt.stats()["last_occlusion_launches"]; pt.Dispose()
        return snaps, n
    want, n1 = _both(run)
    assert n1 == 2                                                   # one per batch: the flavour really ran
    o = oracle_mod.OraclePathTracer(soup, W, H); o.set_camera(cam); configs.apply_settings(o.settings, dict(RayDepth=depth))
    for i in range(2):
        for _ in range(batch):
            o.render()
        assert want[i]["image"] == bits(o.image(0)).tobytes() and want[i]["rays"] == o.rays().tobytes() and want[i]["queue"] == o.alive_queue().tobytes()
        assert want[i]["rays_traced_after"] == o.stats()["rays_traced"]
    o.close()


def test_a_row_that_is_no_multiple_of_the_wave(soup):
    w, h = 33, 17
    cam = _cam("inside", w, h)

    def run(occl):
        pt = _pt(soup, cam, occl, w, h, batch=3, opts=ELIGIBLE, RayDepth=2)
        snaps = []
        for _ in range(2):
            for _ in range(3):
                pt.Compute()
            snaps.append(_snap(pt))
        n = pt.stats()["last_occlusion_launches"]; pt.Dispose()
        return snaps, n
    assert _both(run)[1] == 2


@pytest.mark.parametrize("between", ["nothing", "batch", "max_batch", "update", "dropped"])
@pytest.mark.parametrize("depth,batch", [(2, 9), (3, 2)])
def test_demand_after_the_fact(soup, between, depth, batch):
    """The frame is read first; ray state and queue are asked for afterwards, with a call in between that completes the deferred part (a change of the batch size, a scene
    update) or one that replaces or drops it (further batches)."""
    cam = _cam("inside")
    opts = dict(ELIGIBLE, bounce_pixel_major=2)

    def run(occl):
        pt = _pt(soup, cam, occl, batch=batch, opts=opts, RayDepth=depth)
        snaps = []
        for _ in range(batch):
            pt.Compute()
        snaps.append(_snap(pt, state=False))
        rounds = {"batch": 1, "dropped": 3}.get(between, 0)
        for _ in range(rounds):                                       # the batch before is never asked for: its continuation is dropped
            for _ in range(batch):
                pt.Compute()
            snaps.append(_snap(pt, state=False))
        if between == "max_batch":
            pt.set_max_batch(batch)                                   # (the same size: the call completes the deferred part and keeps the buffers; another size re-allocates them, state and queue are gone then)
        if between == "update":
            mats = soup.materials.copy(); mats["EmissiveFactor"][:] = (3.0, 2.0, 1.0)
            pt.UpdateBuffer(T.IDKPT_BUF_MATERIALS, mats)               # every surface emits from now on; the frame before was traced without
        snaps.append(_snap(pt))
        n = pt.stats()["last_occlusion_launches"]
        for _ in range(batch):                                        # and the library goes on as if nothing had happened
            pt.Compute()
        snaps.append(_snap(pt))
        pt.Dispose()
        return snaps, n
    n1 = _both(run)[1]
    assert n1 == 1 + {"batch": 1, "dropped": 3}.get(between, 0)


def _absurd_soup(native_builder):
    """Two kinds of surface, shuffled through one BLAS.  OPAQUE: a base-colour texel of 1e30 (the finite texel of tests/adversarial_surfaces.py's non_finite swatches — there it
    sits in the emission, which would make the scene ineligible): two such hits and the throughput is infinite; no emission — a hit with an infinite throughput makes the
    radiance NaN (0 x inf).  CUT: alpha 0.25 against a cutoff of 0.5 (its alpha_edges swatches' test, away from the edge: the texel goes through a bilinear mix) — ShadeHit
    returns before it touches the radiance.  So what k_shade_last leaves in the FRAME for a ray whose throughput is not finite depends on WHICH triangle its hit
    record names: the closest, or another one the ray meets."""
    tp = S.soup_triangles(4000, seed=11, extent=2.0, edge=0.6)          # long triangles: many rays meet several, and leaves overlap
    rng = np.random.default_rng(3)
    cut = rng.uniform(0, 1, len(tp)) < 0.5
    meshes = []
    for sel, mat, tex in ((~cut, S.make_material((0.8, 0.8, 0.8, 1.0)), 1), (cut, S.make_material((0.8, 0.8, 0.8, 1.0), alpha_cutoff=0.5), 2)):
        p, i, nrm, tan = S.flat_shaded(tp[sel])
        mat["BaseColorTexture"] = tex
        meshes.append(S.MeshInput(p, i, mat, nrm, tan, uvs=rng.uniform(0, 1, (len(p), 2)).astype(np.float32)))
    sc = S.assemble([{"meshes": meshes}], native_builder, sky_color=(1.0, 1.0, 1.0))
    sc.textures = [np.full((2, 2, 4), 1e30, np.float32), np.full((2, 2, 4), (1.0, 1.0, 1.0, 0.25), np.float32)]
    return sc


def test_throughput_that_is_not_finite_keeps_its_closest_hit(native_builder):
    """k_shade_last runs ShadeHit on the real hit record of a ray whose throughput is not finite: such rays are marked by the kernel that writes their trace-ready record and walk
    closest-hit inside the hit-or-miss launch.  In this scene the frame shows it: a marked ray that stopped at its first accepted triangle instead would, wherever that triangle
    is of the other kind than the closest one, leave NaN where option 0 leaves a finite radiance, or the reverse — and the frame is read before anything re-traces the bounce.
    That both kinds of closest hit exist among those rays is read from option 0: a ray that enters the last bounce with an infinite (not NaN) throughput and a finite radiance
    comes out with NaN (closest hit opaque), with its radiance untouched (closest hit cut), or with inf (miss: sky x inf)."""
    sc = _absurd_soup(native_builder); w, h = W, H; cam = _cam("inside")
    depth = 3                                                        # two opaque hits: the throughput entering bounce 2 is infinite, the radiance still finite
    pre = _pt(sc, cam, 0, w, h, opts=ELIGIBLE, RayDepth=depth - 1, DoRussianRoulette=0)
    pre.Compute(); before = pre.rays().copy(); entering = pre.alive_queue().copy(); pre.Dispose()

    def run(occl):
        pt = _pt(sc, cam, occl, w, h, opts=ELIGIBLE, RayDepth=depth, DoRussianRoulette=0)
        pt.Compute()
        first = _snap(pt); rays = pt.rays().copy()
        pt.Compute(); pt.Compute()
        snaps = [first, _snap(pt, state=False), _snap(pt)]
        n = pt.stats()["last_occlusion_launches"]; pt.Dispose()
        run.rays = rays if occl == 0 else run.rays
        return snaps, n
    run.rays = None
    n1 = _both(run)[1]
    assert n1 == 3
    thr = before["Throughput"][entering]; rad0 = before["Radiance"][entering]; rad1 = run.rays["Radiance"][entering]
    odd = np.isinf(thr).any(axis=1) & ~np.isnan(thr).any(axis=1) & np.isfinite(rad0).all(axis=1)
    closest_opaque = int((odd & np.isnan(rad1).any(axis=1)).sum())
    closest_cut = int((odd & (rad1.view(np.uint32) == rad0.view(np.uint32)).all(axis=1)).sum())
    print("rays entering the last bounce:", len(entering), "with an infinite throughput and a finite radiance:", int(odd.sum()), "closest hit opaque:", closest_opaque, "closest hit cut:", closest_cut)
    assert closest_opaque >= 1 and closest_cut >= 1


@pytest.mark.parametrize("case", ["counters", "emissive", "lights", "defer_last_0", "versions", "split", "fused"])
def test_ineligible_paths_keep_the_closest_hit_launch(soup, native_builder, case):
    """... and are what they were, byte for byte"""
    cam = _cam("inside"); depth = 2; batch = 2
    sc = soup; ov = dict(RayDepth=depth); opts = dict(ELIGIBLE)
    if case == "emissive":
        sc = S.soup_scene(3000, native_builder, seed=7, extent=2.0); sc.materials["EmissiveFactor"][:] = (0.5, 0.25, 0.125)
    if case == "lights":
        sc = S.soup_scene(3000, native_builder, seed=7, extent=2.0); sc.lights = S.make_lights([((0.0, 0.5, -1.0), 0.3, (20.0, 20.0, 20.0))]); ov["DoTraceLights"] = 1
    if case == "defer_last_0":
        opts["defer_last"] = 0
    if case == "split":
        opts["split"] = 2
    if case == "fused":
        opts["fused"] = 2

    def run(occl):
        pt = _pt(sc, cam, occl, batch=batch, opts=opts, **ov)
        if case == "counters":
            pt.enable_counters(True)
        if case == "versions":
            nskin = len(sc.vertex_positions)
            un = np.zeros(nskin, T.GpuUnskinnedVertex)
            un["Position"] = sc.vertex_positions; un["Normal"] = sc.vertices["Normal"]; un["Tangent"] = sc.vertices["Tangent"]; un["JointWeights"][:, 0] = 1.0
            pt.UploadUnskinnedVertices(un); pt.SetSceneVersions(2)
        snaps = []
        for r in range(2):
            pt.Compute()
            if case == "versions":                                    # the batch's second sample sees the geometry moved
                joints = np.zeros((1, 3, 4), np.float32); joints[0, :, :3] = np.eye(3); joints[0, :, 3] = (0.1 * (r + 1), 0.05, -0.2)
                pt.UpdateBuffer(T.IDKPT_BUF_JOINT_MATRICES, joints); pt.Skin(0, 0, 0, nskin); pt.RefitBlas(0)
            pt.Compute()
            snaps.append(_snap(pt))
        st = pt.stats(); pt.Dispose()
        if case == "counters":
            snaps.append({"node_pair_visits": st["node_pair_visits"], "triangle_tests": st["triangle_tests"]})
        return snaps, st["last_occlusion_launches"]
    assert _both(run)[1] == 0
