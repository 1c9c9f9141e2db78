"""Every traversal walk against the CPU oracle on ADVERSARIAL rays (tests/adversarial_rays.py; tests/test_adversarial_rays_ref.py proves on the CPU that the classes are what they
claim): zero and subnormal direction components, origins on node planes (0 * inf = NaN slabs), exact ties, origins on a surface, MaxDist at / one ulp around the hit distance.
Everything is compared on bytes; there is no tolerance in this file.
  3a  idkptTraceRays under every developer option that reaches a query kernel, each set alone from the default: the header promises bit-identical output under all of them
  3b  the path tracer with cameras whose primary rays are all parallel (every 1/dir non-finite) or all in one plane (dir.x == 0 exactly), per-frame data pushed as raw bytes
  3c  the flagged-ray counters after those renders: the vouching walks' `1/dir is not finite -> exact kernel` branches really ran
"""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import configs  # noqa: E402
import adversarial_rays as A  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import assert_equal  # noqa: E402

pytestmark = pytest.mark.gpu

# one option at a time from the default (idkptSetDeveloperOption) ...
VARIANTS = [("default", {})] + [(f"{o}{v}", {o: v}) for o, v in (("query_scheduler", 0), ("query_scheduler", 1), ("pair_nodes", 0), ("pair_nodes", 1), ("split", 0), ("split", 2), ("split", 3),
                                                                   ("force_generic", 1), ("leaf_pool", 7), ("inst_sieve", 0), ("inst_sieve", 8), ("leaf_min", 1), ("leaf_min", 64), ("adv_min", 1),
                                                                   ("grab_unit_log2", 6))]
# ... and the sieved exact loop made to serve closest-hit queries on the lattice's instances, which overlap on purpose (walk_plan.hpp: the sieve and the own TLAS ask for little overlap by default)
VARIANTS += [("sieve_any_overlap", {"inst_sieve": 8, "inst_sieve_overlap": 100}), ("own_tlas_any_overlap", {"inst_tlas": 8, "inst_tlas_overlap": 100}),
             ("sieve_any_overlap_adv1_unit6", {"inst_sieve": 2, "inst_sieve_overlap": 100, "adv_min": 1, "grab_unit_log2": 6})]


@pytest.fixture(scope="module")
def data(native_builder, oracle_mod):
    """per scene: the scene, its batch, and a cache of the oracle's answers on the whole batch (a ray's answer does not depend on its batch: the ragged batches index into it)"""
    out = {}
    for name in A.SCENES:
        sc = A.make_scene(name, native_builder)
        if name == "lattice":            # a light sphere centred on a lattice point: axis rays graze and pierce it
            sc.lights = S.make_lights([((0.25, 0.25, 0.25), 0.125, (9.0, 8.0, 7.0)), ((-0.5, 0.0, 0.5), 0.0625, (2.0, 3.0, 4.0))])
        rays, cls, kinds = A.make_rays(name, sc, lambda r, sc=sc: oracle_mod.trace_rays(sc, r))
        out[name] = {"sc": sc, "rays": rays, "cls": cls, "kinds": kinds, "batches": A.batches(rays, cls), "ref": {}}
    return out


def _want(oracle_mod, d, use_tlas, any_hit, lights):
    key = (use_tlas, any_hit, lights)
    if key not in d["ref"]:
        d["ref"][key] = oracle_mod.trace_rays(d["sc"], d["rays"], any_hit=any_hit, trace_lights=lights, use_tlas=bool(use_tlas))
    return d["ref"][key]


@pytest.mark.parametrize("label,options", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("name", A.SCENES)
def test_queries_equal_the_oracle_under_every_option(oracle_mod, data, name, label, options):
    """idkptTraceRays == the oracle's TraceRay / TraceRayAny, every field of every ray, closest and any hit, instance loop and TLAS, the whole batch (about 13 500 rays over one-wave
    workgroups: the persistent scheduler refills) and the ragged batches of 4 099, 65, 63 and 1 rays.  Every variant is held to the same stored answer, so all variants of one
    (scene, batch) also equal each other.  A failure names the first differing ray: its class, origin, direction and the first differing field."""
    from idkengine_amd.pathtracer import PathTracer
    d = data[name]
    pt = PathTracer(8, 8)
    for k, v in options.items():
        pt.set_option(k, v)
    pt.UploadScene(d["sc"])
    try:
        for use_tlas in ((0, 1) if len(d["sc"].tlas_nodes) else (0,)):
            pt.UseTlas = use_tlas
            for any_hit in (False, True):
                for lights in ((False, True) if name == "lattice" else (False,)):
                    want = _want(oracle_mod, d, use_tlas, any_hit, lights)
                    for bname, idx in d["batches"].items():
                        if lights and bname not in ("all", "65"):
                            continue
                        got = pt.TraceRays(d["rays"][idx], any_hit=any_hit, trace_lights=lights)
                        diff = A.first_difference(got, want[idx], d["rays"][idx], d["cls"][idx], d["kinds"][idx])
                        assert diff is None, f"{name} {label} UseTlas={use_tlas} any_hit={any_hit} lights={lights} batch {bname}: {diff}"
    finally:
        pt.Dispose()


@pytest.mark.parametrize("label,options", VARIANTS + [("sieve_from_2", {"inst_sieve": 2, "inst_sieve_overlap": 100}), ("own_tlas_from_2", {"inst_tlas": 2, "inst_tlas_overlap": 100})],
                         ids=[v[0] for v in VARIANTS] + ["sieve_from_2", "own_tlas_from_2"])
def test_the_strict_root_test_of_the_loop_is_kept(native_builder, oracle_mod, label, options):
    """A.stale_root_scene: a ray meets an instance's (stale) root box at t1 == T exactly.  The loop's root test is strict (BVHIntersect.glsl:32-39): the instance is not entered and
    the triangle that lies in front of its box is not found.  Every query kernel must say the same — the sieved exact loop in particular, which two of the variants put in charge
    of this two-instance scene."""
    from idkengine_amd.pathtracer import PathTracer
    sc = A.stale_root_scene(native_builder); rays = A.stale_root_rays()
    cls = np.full(len(rays), A.CID["regression"]); kinds = np.full(len(rays), -1)
    pt = PathTracer(8, 8)
    for k, v in options.items():
        pt.set_option(k, v)
    pt.UploadScene(sc)
    try:
        for use_tlas in (0, 1):
            pt.UseTlas = use_tlas
            for any_hit in (False, True):
                want = oracle_mod.trace_rays(sc, rays, any_hit=any_hit, use_tlas=bool(use_tlas))
                diff = A.first_difference(pt.TraceRays(rays, any_hit=any_hit), want, rays, cls, kinds)
                assert diff is None, f"{label} UseTlas={use_tlas} any_hit={any_hit}: {diff}"
    finally:
        pt.Dispose()


# ---------------------------------------------------------------------------------------------------------------- 3b / 3c: the path tracer
# ViewPos.x = x0: a node plane of the scene (A.rare_plane; lattice_inst: 1/4, a plane of many nodes of its turned instances)
CAMERAS = {
    # every primary ray is (0, 0, -1) from one point whose x lies on a node plane: 1/dir = (+-inf, +-inf, -1) and 0 * inf slabs
    "parallel": lambda x0: A.perframe("parallel", None, (x0, 0.09375, 1.5)),
    # InvView an exact quarter turn: the rays run along an axis of the world that is not the camera's; off the planes
    "parallel_turned": lambda x0: A.perframe("parallel", A.exact_rotation(1, 1), (1.5, 0.09375, 0.15625)),
    # dir.x == 0 exactly, y / z fan out; ViewPos.x on a node plane
    "planar": lambda x0: A.perframe("planar", None, (x0, 0.1, 1.6), fov=0.8),
    # ... and from outside the scene's slab in x: every ray misses, the tiles' pyramids are flat (k_classify_tiles' degenerate sides and its one-face sky decision)
    "planar_outside": lambda x0: A.perframe("planar", None, (1.75, 0.1, 1.6), fov=0.8),
    # lattice_inst only: between the instances at x = 4 and x = 8, inside the box of the TLAS node that holds both — a ray that is taken and meets no instance
    "parallel_gap": lambda x0: A.perframe("parallel", None, (6.03125, 0.09375, 1.5)),
}


def _camera(cam, name, sc):
    return CAMERAS[cam](0.25 if name == "lattice_inst" else A.rare_plane(sc, 0))


@pytest.fixture(scope="module")
def scenes(native_builder):
    return {name: A.make_scene(name, native_builder) for name in ("lattice", "lattice_inst", "lattice_same_space")}


def _render(oracle_mod, sc, pf, w, h, options, ov, batch=0):
    """the frame on the GPU (developer options set one by one, per-frame data as raw bytes) and in the oracle (the same bytes), compared like the parity tests; returns the GPU's statistics"""
    from idkengine_amd.pathtracer import PathTracer
    o = oracle_mod.OraclePathTracer(sc, w, h); o.set_perframe_data(pf)
    configs.apply_settings(o.settings, ov); o.enable_counters(True); o.render()
    pt = PathTracer(w, h, settings=configs.apply_settings(T.Settings.default(), ov))
    try:
        for k, v in options.items():
            pt.set_option(k, v)
        pt.UploadScene(sc); pt.SetPerFrameData(pf)
        pt.enable_counters(False); pt.enable_primary_hit_capture(True)
        if batch:
            pt.set_max_batch(batch)
        pt.Compute(); pt.flush()
        assert_equal(pt, o, counters=False)      # (visit counters: own-TLAS, unified, wide and packet walks do not reproduce them; the counting build is tested elsewhere)
        return pt.stats()
    finally:
        pt.Dispose(); o.close()


def _enters_root(oracle_mod, sc, pf):
    """RayBoxIntersect(root of BLAS 0) && t1 < FLT_MAX for the one ray of a "parallel" record, with the oracle's own expression (single-BLAS scenes, identity transform)"""
    o = np.ascontiguousarray(pf["ViewPos"][0], np.float32); d = np.ascontiguousarray(A.primary_direction(pf)); root = sc.blas_nodes[1]
    mn = np.ascontiguousarray(root["Min"]); mx = np.ascontiguousarray(root["Max"]); t1 = C.c_float()
    hit = oracle_mod.lib().ref_ray_box(o.ctypes.data, d.ctypes.data, mn.ctypes.data, mx.ctypes.data, C.byref(t1))
    return bool(hit) and t1.value < 3.4028235e+38


FRAMES = [(64, 64, 1), (96, 40, 2)]
LATTICE_OPTIONS = [("packet0", {"packet": 0}, 3), ("packet2", {"packet": 2}, 3), ("wide1", {"wide": 1}, 3), ("fused2", {"fused": 2}, 2), ("tile_cull", {"no_tile_cull": 0}, 3), ("no_tile_cull", {"no_tile_cull": 1}, 3)]


@pytest.mark.parametrize("w,h,spp", FRAMES, ids=["64x64", "96x40x2"])
@pytest.mark.parametrize("label,options,depth", LATTICE_OPTIONS, ids=[c[0] for c in LATTICE_OPTIONS])
@pytest.mark.parametrize("cam", ["parallel", "parallel_turned", "planar", "planar_outside"])
def test_one_blas_frames_equal_the_oracle(oracle_mod, scenes, cam, label, options, depth, w, h, spp):
    """lattice (one BLAS, PreSplit fragments) under the plain / fast walk, the forced packet walk, the wide walk, the fused kernel and with / without the tile classification:
    image, ray records, alive queue, primary hits == the oracle's, bit for bit.
    The flag counters (3c), as include/idkpt.h defines them: PacketFlaggedRays / WideFlaggedRays count the rays the walk did not vouch for, whatever the reason; a ray only reaches
    these walks if its root-box test passed (k_gen_primary culls the others before any launch).  The packet walk is the primary launch only, so with a parallel camera — every
    primary ray the same ray, its 1/dir non-finite — the counter is exactly the number of primary rays if that ray enters the root box, else 0.  The wide walk also traces the
    bounces, whose rays it flags for its other reasons too: there the primary rays are a lower bound (the exact count is asserted at RayDepth 1 below)."""
    sc = scenes["lattice"]; pf = _camera(cam, "lattice", sc)
    st = _render(oracle_mod, sc, pf, w, h, options, dict(RayDepth=depth, SamplesPerPixel=spp))
    if cam.startswith("parallel"):
        primary = w * h * spp * int(_enters_root(oracle_mod, sc, pf))
        assert primary > 0                                                  # (the cameras above are chosen to enter)
        if label == "packet2":
            assert st["packet_packets"] > 0 and st["packet_flagged_rays"] == primary and st["packet_rays_entered"] == 0, st
        if label == "wide1":
            assert st["wide_flagged_rays"] >= primary, st
    if label == "packet0":
        assert st["packet_packets"] == 0 and st["packet_flagged_rays"] == 0 and st["wide_flagged_rays"] == 0, st


@pytest.mark.parametrize("cam", ["parallel", "parallel_turned"])
def test_the_wide_walk_hands_over_exactly_the_non_finite_primary_rays(oracle_mod, scenes, cam):
    """RayDepth 1: the primary launch is the only one, every ray that reaches it has a non-finite 1/dir: WideFlaggedRays == the number of primary rays (the ray enters the root box)."""
    sc = scenes["lattice"]; pf = _camera(cam, "lattice", sc); w, h, spp = 96, 40, 2
    assert _enters_root(oracle_mod, sc, pf)
    st = _render(oracle_mod, sc, pf, w, h, {"wide": 1}, dict(RayDepth=1, SamplesPerPixel=spp))
    assert st["wide_flagged_rays"] == w * h * spp, st


def test_eight_samples_in_one_batch_reach_the_pixel_major_list(oracle_mod, scenes):
    """8 samples per pixel traced as one batch: the primary list is pixel-major and option packet = 1 (the default) lets the packet walk take the first launch by measurement;
    planar camera, so every ray of every packet has dir.x == 0 and is handed to the exact kernel if it enters the root box."""
    sc = scenes["lattice"]; w, h = 64, 64
    for cam in ("planar", "parallel"):
        st = _render(oracle_mod, sc, _camera(cam, "lattice", sc), w, h, {"packet": 1}, dict(RayDepth=3, SamplesPerPixel=8), batch=8)
        assert st["packet_packets"] > 0 and st["packet_flagged_rays"] > 0 and st["packet_rays_entered"] == 0, st


INST_OPTIONS = [("own_tlas", {"inst_tlas": 8, "inst_tlas_overlap": 100, "inst_unify": 0}, 0), ("loop", {"inst_tlas": 0}, 0), ("use_tlas", {"inst_tlas": 8}, 1)]


@pytest.mark.parametrize("w,h,spp", FRAMES, ids=["64x64", "96x40x2"])
@pytest.mark.parametrize("label,options,use_tlas", INST_OPTIONS, ids=[c[0] for c in INST_OPTIONS])
@pytest.mark.parametrize("cam", ["parallel", "parallel_turned", "planar", "parallel_gap"])
def test_instanced_frames_equal_the_oracle(oracle_mod, scenes, cam, label, options, use_tlas, w, h, spp):
    """lattice_inst (13 instances, exact quarter turns, a doubled instance, one general rotation) through the library's own TLAS (inst_tlas_overlap 100: its instances overlap on
    purpose), through the exact loop / its sieve, and through the host's TLAS.
    InstTlasFlaggedRays (include/idkpt.h): the rays the own-TLAS walk did not vouch for.  Primary rays that miss both children of the own TLAS's root are culled before the launch
    (k_gen_primary) and never counted; a ray the walk takes is flagged at once if a component of its world 1/dir is not finite.  Parallel cameras (every primary ray the same ray,
    kept — it runs inside a box of the tree): at least the primary rays; RayDepth 1 below asserts the exact count."""
    sc = scenes["lattice_inst"]; pf = _camera(cam, "lattice_inst", sc)
    st = _render(oracle_mod, sc, pf, w, h, options, dict(RayDepth=3, SamplesPerPixel=spp, UseTlas=use_tlas))
    if label == "own_tlas":
        assert st["inst_tlas_flagged_rays"] >= (w * h * spp if cam.startswith("parallel") else 1), st
    else:
        assert st["inst_tlas_flagged_rays"] == 0, st


@pytest.mark.parametrize("cam", ["parallel", "parallel_gap"])
def test_the_own_tlas_walk_hands_over_exactly_the_non_finite_primary_rays(oracle_mod, scenes, cam):
    """RayDepth 1, parallel camera: InstTlasFlaggedRays == the number of primary rays — also for the ray that passes BETWEEN two instances inside the box of the node that holds
    both ("parallel_gap"): it meets no instance, so only the world ray's own `1/dir is not finite` test (kernels_trace_inst.hpp, where a lane takes a ray) can hand it over."""
    sc = scenes["lattice_inst"]; w, h, spp = 96, 40, 2
    st = _render(oracle_mod, sc, _camera(cam, "lattice_inst", sc), w, h, {"inst_tlas": 8, "inst_tlas_overlap": 100, "inst_unify": 0}, dict(RayDepth=1, SamplesPerPixel=spp))
    assert st["inst_tlas_flagged_rays"] == w * h * spp, st


@pytest.mark.parametrize("w,h,spp", FRAMES, ids=["64x64", "96x40x2"])
@pytest.mark.parametrize("unify", [4096, 0])
@pytest.mark.parametrize("cam", ["parallel", "parallel_turned", "planar"])
def test_same_space_frames_equal_the_oracle(oracle_mod, scenes, cam, unify, w, h, spp):
    """lattice_same_space (12 BLASes under one InvModel) through the unified tree with the packet walk forced on its primary launch, and with the unified tree switched off.
    Unified walks count their flagged rays in InstTlasFlaggedRays, the packet launch in PacketFlaggedRays; the unified packet walk skips the root tests, so with a parallel camera
    every primary ray enters and is handed over: PacketFlaggedRays == the number of primary rays."""
    sc = scenes["lattice_same_space"]; pf = _camera(cam, "lattice_same_space", sc)
    st = _render(oracle_mod, sc, pf, w, h, {"inst_unify": unify, "packet": 2}, dict(RayDepth=3, SamplesPerPixel=spp))
    if unify:
        assert st["inst_unified_launches"] > 0 and st["packet_packets"] > 0, st
        if cam.startswith("parallel"):
            assert st["packet_flagged_rays"] == w * h * spp, st
    else:
        assert st["inst_unified_launches"] == 0 and st["packet_packets"] == 0, st
