"""State-machine check of everything the library derives from what the host uploads (runs late, just before test_gpu_zz_random_api.py and for that file's reason: a failure here must
not hide the other files under pytest -x).  Random sequences of geometry updates (tests/update_sequences.py) on several-instance scenes: no stale paired layout, instance record, own
TLAS, unified tree, triangle mark, wide node or packet state may show in what a host reads."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import configs  # noqa: E402,F401
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import bits  # noqa: E402
import update_sequences as U  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("IDKPT_UPDATE_SEQUENCE_SEEDS", str(U.DEFAULT_SEEDS)))
WALKS = ("own_tlas", "unified", "packet", "sieve", "loop", "tlas")
_REACH = {"default": {}, "forced": {}}                   # forcing -> seed -> the walks that were seen to run on the product context
_COUNTERS = ("inst_unified_launches", "packet_packets", "inst_tlas_flagged_rays")   # (+ inst_unified_entries, a level and not a total: read with them)
_PLAIN = (("defer_last", 0), ("inst_tlas", 0), ("inst_unify", 0), ("inst_sieve", 0), ("inst_general", 0), ("packet", 0), ("wide", 0), ("query_scheduler", 0))


@pytest.fixture(scope="module")
def scenes(native_builder):
    return U.build_scenes(native_builder)


class _Probe:
    """Which walks run, read from a THIRD context: configured like the product context A and handed every call A gets, but never compared with anything.  idkptGetStats launches what
    is queued, so reading it on A between a queued idkptRender and an update would move that launch in front of the update call — the order the file is there to test.  On the probe
    the statistics are read around every frame: launches on the unified tree and its entries, packets, and the rays a tree walk handed to the exact loop (inst_tlas_flagged_rays: with
    no unified launch in the same frame they are the own TLAS's, so an own-TLAS frame that flags nothing goes unseen).  The statistics have NO counter for the sieve, the instance loop
    or the TLAS walk.  Those three are inferred from the state walk_plan.hpp gives them, with what the counters can say asserted: loop = a frame of several instances at more than one
    scene version, tlas = a frame under UseTlas (every tree counter must stand still over both: optional_walks_allowed); sieve = a closest-hit query on several instances, one scene
    version, no UseTlas, right behind a frame of the probe — rendered for the purpose — that a tree walk was seen to trace (choose_walk sends such a query to the sieve)."""

    def __init__(self, pt):
        self.pt, self.seen, self.last = pt, set(), {k: 0 for k in _COUNTERS}

    def _delta(self):
        st = self.pt.stats(); d = {k: st[k] - self.last[k] for k in _COUNTERS}; self.last = {k: st[k] for k in _COUNTERS}
        return d, st["inst_unified_entries"]

    def frame(self, multi, use_tlas, versions):
        """one idkptRender on the probe and what the counters say of it; True when a tree walk was seen"""
        self._delta(); self.pt.Compute(); d, entries = self._delta()
        if use_tlas or versions > 1:
            assert d == {k: 0 for k in _COUNTERS}, (d, multi, use_tlas, versions)
            self.seen.add("tlas" if use_tlas else ("loop" if multi else "plain"))
            return False
        if d["packet_packets"] > 0:
            self.seen.add("packet")
        if d["inst_unified_launches"] > 0:
            assert multi and entries >= 2, (d, entries)
            self.seen.add("unified"); return True
        if d["inst_tlas_flagged_rays"] > 0:
            assert multi, d
            self.seen.add("own_tlas"); return True
        return False

    def query(self, rays, multi, use_tlas, versions):
        if multi and not use_tlas and versions == 1 and self.frame(multi, use_tlas, versions):
            self.seen.add("sieve")
        return self.pt.TraceRays(rays)


def _same(a, b, where, rays=False):
    assert (bits(a.Result) == bits(b.Result)).all(), where
    assert a.AccumulatedSamples == b.AccumulatedSamples, where
    if rays:
        assert a.rays().tobytes() == b.rays().tobytes(), where
        assert (a.alive_queue() == b.alive_queue()).all(), where


_ORACLE = {}                                             # (seed, step) -> the oracle's frame and hits of the mirror there: computed once, shared by both forcings (the mirror does not depend on them)


def _against_the_oracle(a, b, m, oracle_mod, qseed, where, key):
    """One fresh frame of the product against the CPU oracle's frame of the mirror (and the replay's: it gets the same calls and stays in step), then 512 queries against the oracle's."""
    for p in (a, b):
        p.ResetAccumulation(); p.Compute()
    rays = U.query_rays(qseed)
    if key not in _ORACLE:
        o = m.oracle_frame(oracle_mod)
        try:
            _ORACLE[key] = (bits(o.image(0)).copy(), o.rays().tobytes(), o.alive_queue().copy(), m.oracle_hits(oracle_mod, rays).tobytes())
        finally:
            o.close()
    img, state, alive, hits = _ORACLE[key]
    wrong = {}
    for name, p in (("product", a), ("replay", b)):
        got = bits(p.Result)
        wrong[name] = dict(pixels=int((got != img).any(axis=-1).sum()), rays=p.rays().tobytes() != state, queue=not np.array_equal(p.alive_queue(), alive), hits=p.TraceRays(rays).tobytes() != hits)
    assert not any(v for w in wrong.values() for v in w.values()), (where, wrong)
    _same(a, b, where, rays=True)


def _product(forcing, seed):
    """A context set up as the product context of (forcing, seed)"""
    from idkengine_amd.pathtracer import PathTracer
    a = PathTracer(U.W, U.H)
    orng = np.random.default_rng(9000 + seed)
    a.set_max_batch(int(orng.integers(2, 9)))
    if forcing == "forced":
        for name, v in (("inst_tlas", 2), ("inst_tlas_overlap", 100), ("packet", 2), ("inst_braid", (0, 24, 2048)[seed % 3])):
            a.set_option(name, v)
        # free choices of the implementation, from their own generator: none may show in what a host reads
        for name, values in (("fused", [1, 2, 2, 0]), ("split", [1, 2, 3, 0]), ("wide", [0, 0, 1]), ("wide_cap", [0, 0, 5]), ("leaf_pool", [-1, 7, 0, 1]), ("trace_waves", [0, 0, 1]), ("uni_refill", [16, 32]), ("pair_nodes", [1, 1, 0])):
            a.set_option(name, int(orng.choice(values)))
    return a


def _run(ops, start, forcing, seed, scenes, oracle_mod, oracle_builder, mid=None, reach=None):
    """A (the product) and B (the plain replay) get every op and are compared wherever the sequence reads; nothing else is ever asked of A, so what is queued on it stays queued
    until the library itself launches it.  With `reach`, a third context (_Probe) gets the ops too and says which walks they lead to."""
    from idkengine_amd.pathtracer import PathTracer
    cams = U.cameras()
    m = U.Mirror(scenes, start, oracle_builder)
    a = _product(forcing, seed); b = PathTracer(U.W, U.H); c = _product(forcing, seed) if reach is not None else None
    try:
        for name, v in _PLAIN:
            b.set_option(name, v)
        b.set_max_batch(1)
        everyone = [p for p in (a, b, c) if p is not None]
        for p in everyone:
            p.UploadScene(m.scene); p.SetCamera(cams[0]); p.RayDepth = m.settings["RayDepth"]
        r = _Probe(c) if c is not None else None
        state = lambda: (len(m.scene.blas_instances) > 1, m.settings["UseTlas"], m.versions)   # noqa: E731
        prev = None
        for step, op in enumerate(ops):
            where = (forcing, seed, step, op[0])
            calls = m.apply(op)
            U.play(a, calls, cams, product=True); U.play(b, calls, cams, product=False)
            if r is not None:
                if op[0] == "compute":
                    r.frame(*state())
                else:
                    U.play(c, calls, cams, product=True)
            if op[0] == "read":
                _same(a, b, where)
            elif op[0] == "state" and prev == "compute":
                assert a.rays().tobytes() == b.rays().tobytes(), where
                assert (a.alive_queue() == b.alive_queue()).all(), where
            elif op[0] == "query":
                rays = U.query_rays(op[1])
                got = a.TraceRays(rays).tobytes()
                assert got == b.TraceRays(rays).tobytes(), where
                if r is not None:
                    assert r.query(rays, *state()).tobytes() == got, where
            if step == mid:
                _against_the_oracle(a, b, m, oracle_mod, 500 + seed, where + ("oracle",), (seed, step))
            prev = op[0]
        where = (forcing, seed, "end")
        _same(a, b, where)
        for p in (a, b):                                  # the ray state is only defined right after a sample
            p.Compute()
        _same(a, b, where, rays=True)
        sc = m.scene
        for p in (a, b):
            assert p.DownloadBuffer(T.IDKPT_BUF_VERTEX_POSITIONS, np.float32, 3 * len(sc.vertex_positions)).tobytes() == sc.vertex_positions.tobytes(), where
            assert p.DownloadBuffer(T.IDKPT_BUF_BLAS_NODES, T.GpuBlasNode, len(sc.blas_nodes)).tobytes() == sc.blas_nodes.tobytes(), where
            assert p.DownloadBuffer(T.IDKPT_BUF_MESH_TRANSFORMS, T.GpuMeshTransform, len(sc.mesh_transforms)).tobytes() == sc.mesh_transforms.tobytes(), where
            if m.tlas_built:
                assert p.DownloadBuffer(T.IDKPT_BUF_TLAS_NODES, T.GpuTlasNode, len(sc.tlas_nodes)).tobytes() == sc.tlas_nodes.tobytes(), where
        _against_the_oracle(a, b, m, oracle_mod, 900 + seed, where + ("oracle",), (seed, "end"))
        if r is not None:
            r.frame(*state())
            reach[seed] = r.seen
    finally:
        for p in (a, b, c):
            if p is not None:
                p.Dispose()


@pytest.mark.parametrize("forcing", ["default", "forced"])
@pytest.mark.parametrize("seed", range(SEEDS))
def test_update_sequences_match_plain_replay_and_oracle(scenes, oracle_mod, oracle_builder, seed, forcing):
    """A random sequence of scene updates (partial and whole transform uploads, vertices moved with and without a refit, node patches, TLAS rebuilds, scene swaps, scene versions),
    frames, queries and reads on two contexts — A: the product (forcing = default: as shipped; forced: the own TLAS from two instances on, whatever the overlap, the packet walk on
    every primary launch it may take, re-braiding by seed, and the implementation's free choices drawn at random), B: the plain replay with everything optional switched off (max batch 1,
    one scene version, thread-per-ray queries) — must read the same wherever the host reads; the geometry both hold must be the mirror's, byte for byte; and at one step fixed by the
    seed and at the end a fresh frame and 512 queries must equal the CPU oracle's on the mirror (what would catch A and B sharing a stale structure)."""
    _run(U.sequence(seed), U.start_scene(seed), forcing, seed, scenes, oracle_mod, oracle_builder, mid=8 + seed % 12, reach=_REACH[forcing])


def test_update_behind_a_queued_sample_invalidates_what_its_launch_derived(scenes, oracle_mod, oracle_builder):
    """What the random sequences found, reduced (profiles/update_sequences.md): twelve BLASes in one space, a sample QUEUED (max batch > 1, nothing read), then one transform patched.
    With one scene version the patch has to launch the queued sample first, and that launch derives the unified tree, the own TLAS and the instance records from the transforms that
    are about to be overwritten — and marks them valid.  ver_writable used to invalidate them before that launch instead of behind it, so the next frame and the next queries walked
    the old instances (774 wrong pixels of 6 144) while the plain replay, which derives nothing, was right.  Nothing may be asked of the product context between the frame and the
    patch (no statistics either: idkptGetStats would launch the sample itself), hence no probe here."""
    ops = [("xf_all", ("scale", (1.121, 1.424, 0.534), (0.816, 1.957, 1.302))), ("compute",), ("xf_one", 10, ("shear", (0.169, -0.032), (-0.542, 1.862, -1.906)))]
    for forcing in ("default", "forced"):
        _run(ops, "d", forcing, 10000, scenes, oracle_mod, oracle_builder)


def test_the_sequences_reached_every_walk():
    """Without this the file could pass having walked the instance loop throughout.  (Runs after the sequences; skips when fewer seeds than the default were selected; a default seed
    that left no record — it failed before its end — makes this test fail as not evaluated, never skip.)"""
    if SEEDS < U.DEFAULT_SEEDS:
        pytest.skip("needs every default seed under both forcings")
    missing = {f: sorted(set(range(U.DEFAULT_SEEDS)) - set(_REACH[f])) for f in _REACH}
    assert not any(missing.values()), ("not evaluated: these seeds did not reach their end", missing)
    by_walk = {f: {w: sorted(s for s, seen in _REACH[f].items() if w in seen) for w in WALKS} for f in _REACH}
    print("walks by seed:", by_walk)
    for w in WALKS:
        assert len(by_walk["forced"][w]) >= 3, (w, by_walk["forced"])
    assert len(set(by_walk["default"]["own_tlas"]) | set(by_walk["default"]["unified"])) >= 3, by_walk["default"]
