"""The deterministic companion of tests/test_gpu_zy_update_sequences.py: one case per (cause, walk).  Each derived scene structure (csrc/derived_scene.hpp) is derived by a frame on
the walk that reads it, one cause makes it stale, and the next frame must read as a fresh context reads that was given the final state directly and walks nothing optional.

Scenes: two BLASes of 300 triangles under one sheared matrix (one space: the unified tree), three instances of one BLAS of 400 triangles, two of them under the same matrix (the own
TLAS, the sieve; a BLAS used twice has no unified tree, and the exact ties are what the own TLAS's one counter counts), update_sequences' one BLAS of 3 000 (packets, wide nodes, the
paired layout), and a second scene of each shape for the re-upload.  64 x 36 at RayDepth 2, eight samples a batch, so the primary list is pixel-major.

Which walk ran is read from a THIRD context, as in the update-sequence file and for its reason (statistics launch what is queued): unified launches, packets, wide node visits, and
the rays the own TLAS handed to the exact loop.  The sieve and the paired layout have no counter: the sieve is a closest-hit query right behind a frame a tree walk was seen to trace
(choose_walk sends such a query there), the paired layout is a one-BLAS frame under the defaults with packets and wide nodes off and their counters standing still (walk_plan.hpp: Fast).
A case whose walk is not seen, before the cause or after it, fails.  No (cause, walk) pair is dropped: all thirty reach their walk at this size."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import configs  # noqa: E402,F401
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import bits  # noqa: E402
import update_sequences as U  # noqa: E402
from test_gpu_zy_update_sequences import _PLAIN  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, BATCH = 64, 36, 8
_COUNTERS = ("inst_unified_launches", "packet_packets", "wide_node_visits", "inst_tlas_flagged_rays")
# walk -> (scene, the scene of a re-upload, the options that pin the walk, the inst_* option a case flips — one that leaves the walk what it is)
WALKS = {
    "own_tlas": ("three", "three_x", dict(inst_tlas=2, inst_tlas_overlap=100, inst_unify=0, packet=0), ("inst_braid", 16)),
    "unified": ("two", "two_x", dict(packet=0), ("inst_unify_radius", 4)),
    "sieve": ("three", "three_x", dict(inst_tlas=2, inst_tlas_overlap=100, inst_unify=0, packet=0), ("inst_sieve_overlap", 100)),
    "packet": ("one", "one_x", dict(packet=2), ("inst_tlas", 2)),
    "wide": ("one", "one_x", dict(wide=1, wide_count=1, packet=0), ("inst_sieve", 2)),
    "pair": ("one", "one_x", dict(packet=0), ("inst_general", 2)),
}
# cause -> the ops of update_sequences.Mirror by scene shape (None: the option flip, no call of the mirror's)
CAUSES = {
    "transform": dict(one=[("xf_all", ("rigid", 40.0, (0.3, -0.2, 0.1)))], two=[("xf_all", ("scale", (1.2, 0.8, 1.1), (0.2, 0.1, -0.3)))], three=[("xf_one", 0, ("rigid", 40.0, (0.3, -0.2, 0.1)))]),
    "vertices_refit": dict(one=[("verts", 0, 3, 11), ("refit", 0)], two=[("verts", 1, 3, 12), ("refit", 1)], three=[("verts", 0, 3, 13), ("refit", 0)]),
    "node_rewrite": dict(one=[("verts", 0, 3, 21), ("nodes", 0)], two=[("verts", 1, 3, 22), ("nodes", 1)], three=[("verts", 0, 3, 23), ("nodes", 0)]),
    "scene": dict(one=[("scene", "one_x")], two=[("scene", "two_x")], three=[("scene", "three_x")]),
    "inst_option": None,
}


@pytest.fixture(scope="module")
def scenes(native_builder):
    sh = np.eye(4); sh[0, 1] = 0.35; sh[2, 0] = -0.2
    m = S.rotation_y(33.0) @ np.diag([1.3, 0.8, 1.1, 1.0]) @ sh @ S.translation((0.5, -0.25, 1.0))
    two = lambda seed: S.assemble([U._soup_blas(300, seed + 17 * k, 3.0, 0.35, True, m) for k in range(2)], native_builder)   # noqa: E731
    def three(seed):                                      # one BLAS of 400 triangles three times, instances 1 and 2 under the same matrix: every ray that hits them first is an exact tie, which the own TLAS hands to the exact loop
        sc = S.assemble([U._soup_blas(400, seed, 2.5, 0.3, True)], native_builder, build_tlas=False)
        mats = [np.eye(4), S.rotation_y(30.0) @ S.translation((1.5, 0.0, 0.5)), S.rotation_y(30.0) @ S.translation((1.5, 0.0, 0.5))]
        inst = np.zeros(3, T.GpuBlasInstance); inst["BlasId"] = 0; inst["MeshTransformId"] = np.arange(3)
        sc.blas_instances = inst; sc.mesh_transforms = np.concatenate([S.transform_from_matrix(x) for x in mats])
        S.rebuild_tlas(sc, native_builder)
        return sc
    return {"one": S.soup_scene(3000, native_builder, seed=31, refittable=True, extent=2.5, edge=0.3), "one_x": S.soup_scene(3000, native_builder, seed=47, refittable=True, extent=2.5, edge=0.3),
            "two": two(80), "two_x": two(180), "three": three(40), "three_x": three(140)}


def _context(options):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(W, H)
    pt.set_max_batch(BATCH)
    for name, v in options.items():
        pt.set_option(name, v)
    return pt


def _frame(pt):
    """a fresh accumulation of one batch; everything is launched and read when it returns"""
    pt.ResetAccumulation()
    for _ in range(BATCH):
        pt.Compute()
    pt.flush(); pt.synchronize()


def _seen(probe, walk, rays, where):
    """one frame on the probe (and, for the sieve, the query behind it); fails where the counters do not show the pinned walk"""
    before = probe.stats(); _frame(probe); after = probe.stats()
    d = {k: after[k] - before[k] for k in _COUNTERS}
    print(where, d)
    if walk in ("own_tlas", "sieve"):
        assert d["inst_unified_launches"] == 0 and d["inst_tlas_flagged_rays"] > 0, (where, d)
    elif walk == "unified":
        assert d["inst_unified_launches"] > 0 and after["inst_unified_entries"] >= 2, (where, d)
    elif walk == "packet":
        assert d["packet_packets"] > 0, (where, d)
    elif walk == "wide":
        assert d["wide_node_visits"] > 0 and d["packet_packets"] == 0, (where, d)
    else:
        assert d == {k: 0 for k in _COUNTERS}, (where, d)
    return probe.TraceRays(rays) if walk == "sieve" else None


@pytest.mark.parametrize("cause", list(CAUSES))
@pytest.mark.parametrize("walk", list(WALKS))
def test_a_stale_structure_never_shows(scenes, oracle_builder, walk, cause):
    from idkengine_amd.pathtracer import PathTracer
    start, _, options, flip = WALKS[walk]
    cam = U.cameras(W, H)[0]
    rays = U.query_rays(77)
    m = U.Mirror(scenes, start, oracle_builder)
    a = _context(options); c = _context(options); b = PathTracer(W, H)
    try:
        for p in (a, c):
            p.UploadScene(m.scene); p.SetCamera(cam); p.RayDepth = 2
        # 1. the structure is derived and marked
        _frame(a)
        first = _seen(c, walk, rays, (walk, cause, "before"))
        if walk == "sieve":
            assert a.TraceRays(rays).tobytes() == first.tobytes(), (walk, cause, "before")
        # 2. the cause
        if CAUSES[cause] is None:
            for p in (a, c):
                p.set_option(*flip)
        else:
            for op in CAUSES[cause][start]:
                calls = m.apply(op)
                U.play(a, calls, [cam]); U.play(c, calls, [cam])
        # 3. a fresh accumulation, against a fresh context that got the final state directly and the plain walks
        for name, v in _PLAIN:
            b.set_option(name, v)
        b.set_max_batch(1)
        b.UploadScene(m.scene); b.SetCamera(cam); b.RayDepth = 2
        _frame(a); _frame(b)
        again = _seen(c, walk, rays, (walk, cause, "after"))
        where = (walk, cause)
        assert (bits(a.Result) == bits(b.Result)).all(), where
        assert a.AccumulatedSamples == b.AccumulatedSamples == BATCH, where
        assert a.rays().tobytes() == b.rays().tobytes(), where
        assert (a.alive_queue() == b.alive_queue()).all(), where
        if walk == "sieve":
            hits = b.TraceRays(rays).tobytes()
            assert a.TraceRays(rays).tobytes() == hits and again.tobytes() == hits, where
    finally:
        for p in (a, b, c):
            p.Dispose()
