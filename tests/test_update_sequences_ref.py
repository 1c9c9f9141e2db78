"""tests/update_sequences.py on its own (no GPU): the generator is deterministic, its default seed set contains the transitions the GPU test is there for, and the host mirror survives
every default sequence against the CPU oracle.  This guards the helper, not the library."""
import copy
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
from idkengine_amd import scenes as S  # noqa: E402
import update_sequences as U  # noqa: E402

SEEDS = range(U.DEFAULT_SEEDS)


@pytest.fixture(scope="module")
def scenes(native_builder):
    return U.build_scenes(native_builder)


def test_sequences_are_deterministic_and_well_formed():
    for seed in SEEDS:
        a, b = U.sequence(seed), U.sequence(seed)
        assert a == b and len(a) == U.LENGTH and all(op[0] in U.KINDS for op in a), seed
    assert len({tuple(U.sequence(s)) for s in SEEDS}) == len(SEEDS)


def test_scene_table_matches_the_scenes(scenes):
    for name, info in U.INFO.items():
        sc = scenes[name]
        assert len(sc.blas_instances) == info["instances"] and len(sc.blas_descs) == info["blases"] and len(sc.materials) == info["materials"], name
        assert tuple(int(b) for b in np.nonzero(sc.blas_descs["IsRefittable"])[0]) == info["refittable"], name
        assert len(sc.mesh_transforms) == info["instances"] and len(sc.tlas_nodes) == 2 * info["instances"] - 1, name
        assert 2000 <= len(sc.blas_triangles) <= 5000, name                                  # "a few thousand triangles each"
        if info["blases"] > 1:
            assert any(b > 0 for b in info["refittable"]) and sc.blas_descs["NodeOffset"][max(info["refittable"])] > 0, name
    xf = scenes["d"].mesh_transforms
    assert all(xf[i].tobytes() == xf[0].tobytes() for i in range(len(xf)))                   # (d) is one space ...
    assert scenes["e"].mesh_transforms[1].tobytes() == scenes["e"].mesh_transforms[4].tobytes() and scenes["e"].blas_instances["BlasId"][1] == scenes["e"].blas_instances["BlasId"][4]   # ... (e) has its tie


def _trace(seed):
    """(op, scene name before it, scene name after it, versions after it, use_tlas after it) along a sequence"""
    name, ver, tl, out = U.start_scene(seed), 1, 0, []
    for op in U.sequence(seed):
        before = name
        if op[0] == "scene":
            name = op[1]
        elif op[0] == "versions":
            ver = op[1]
        elif op[0] == "use_tlas":
            tl = op[1]
        out.append((op, before, name, ver, tl))
    return out


def _run(tr, i, kinds):
    """ops i, i + 1, ... are of these kinds (contiguous)"""
    return i + len(kinds) <= len(tr) and all(tr[i + j][0][0] == k for j, k in enumerate(kinds))


def _transitions(seed):
    tr = _trace(seed); found = set()
    for i, (op, before, after, ver, tl) in enumerate(tr):
        if _run(tr, i, ("xf_all", "compute", "xf_one", "compute")) and U.INFO[before]["instances"] > 1:
            found.add("one_space_then_out")
        if _run(tr, i, ("xf_one", "compute", "xf_all", "compute")) and U.INFO[before]["instances"] > 1:
            found.add("back_into_one_space")
        if op == ("versions", 3):
            j = next((j for j in range(i + 1, len(tr)) if tr[j][0][0] == "versions"), None)
            if j is not None and tr[j][0] == ("versions", 1) and any(tr[m][0][0] == "compute" for m in range(i + 1, j)) and _run(tr, j + 1, ("compute",)):
                found.add("versions_3_then_1")
        if op[0] == "scene" and U.INFO[op[1]]["instances"] >= 8:
            j = next((j for j in range(i + 1, len(tr)) if tr[j][0][0] == "scene"), None)
            m = None if j is None else next((m for m in range(j + 1, len(tr)) if tr[m][0][0] == "scene"), None)
            if m is not None and U.INFO[tr[j][0][1]]["instances"] == 1 and U.INFO[tr[m][0][1]]["instances"] >= 8 and all(any(tr[q][0][0] == "compute" for q in range(lo, hi)) for lo, hi in ((i, j), (j, m))):
                found.add("many_one_many")
        if _run(tr, i, ("refit", "compute")) and op[1] > 0:
            found.add("refit_beyond_blas_0")
        if _run(tr, i, ("verts", "compute", "refit", "compute")) and tr[i + 2][0][1] == op[1]:
            found.add("stale_then_refitted")
        if _run(tr, i, ("nodes", "compute")):
            found.add("nodes_then_compute")
    return found


def test_default_seeds_contain_every_op_and_every_transition():
    count = {k: 0 for k in U.KINDS}
    for seed in SEEDS:
        for op in U.sequence(seed):
            count[op[0]] += 1
    assert min(count.values()) >= 10, count
    assert count["compute"] > max(v for k, v in count.items() if k != "compute"), count                  # compute is the commonest op
    seen = {}
    for seed in SEEDS:
        for t in _transitions(seed):
            seen.setdefault(t, []).append(seed)
    for t in ("one_space_then_out", "back_into_one_space", "versions_3_then_1", "many_one_many", "refit_beyond_blas_0", "stale_then_refitted", "nodes_then_compute"):
        assert len(seen.get(t, [])) >= 3, (t, seen)
    # what the GPU file's reach test needs the sequences to offer: frames through the TLAS, and frames of several instances at three scene versions (the instance loop), in three seeds each
    tlas = [s for s in SEEDS if any(op[0] == "compute" and tl for op, _, _, _, tl in _trace(s))]
    loop = [s for s in SEEDS if any(op[0] == "compute" and not tl and ver > 1 and U.INFO[after]["instances"] > 1 for op, _, after, ver, tl in _trace(s))]
    query = [s for s in SEEDS if any(op[0] == "query" and not tl and ver == 1 and U.INFO[after]["instances"] > 1 for op, _, after, ver, tl in _trace(s))]
    assert len(tlas) >= 3 and len(loop) >= 3 and len(query) >= 3, (tlas, loop, query)
    # every op's arguments fit the scene it meets
    for seed in SEEDS:
        for op, before, after, ver, tl in _trace(seed):
            info = U.INFO[before]
            if op[0] == "xf_one":
                assert 0 <= op[1] < info["instances"]
            elif op[0] == "xf_range":
                assert 1 <= len(op[2]) <= 3 and 0 <= op[1] and op[1] + len(op[2]) <= info["instances"]
            elif op[0] == "refit":
                assert op[1] in info["refittable"]
            elif op[0] in ("verts", "nodes"):
                assert 0 <= op[1] < info["blases"]
            elif op[0] == "material":
                assert 0 <= op[1] < info["materials"]


@pytest.mark.parametrize("seed", SEEDS)
def test_mirror_alone_against_the_oracle(scenes, oracle_mod, oracle_builder, native_builder, seed):
    """Every default sequence on the mirror only: after each geometry op the oracle renders the mirror (one bounce: this is about the helper's arrays being a scene) and the arrays keep
    their shapes.  The mirror's TLAS is rewritten by a `tlas` op or a scene swap only, as the device's is: after a transform, vertex or node op it is stale on purpose, on both sides,
    so "equals rebuild_tlas of the mirror" is asserted while no box or transform has moved since it was built — against a rebuild of a copy by the OTHER builder (the mirror builds with
    the oracle's, the copy with the library's host builder), which is not the same code run twice."""
    m = U.Mirror(scenes, U.start_scene(seed), oracle_builder)
    pristine = {k: v.vertex_positions.copy() for k, v in scenes.items()}
    for op in U.sequence(seed):
        shape = None if op[0] == "scene" else (len(m.scene.blas_nodes), len(m.scene.vertex_positions), len(m.scene.mesh_transforms), len(m.scene.tlas_nodes))
        calls = m.apply(op)
        assert isinstance(calls, list)
        if op[0] not in U.GEOMETRY:
            continue
        if shape is not None:
            assert shape == (len(m.scene.blas_nodes), len(m.scene.vertex_positions), len(m.scene.mesh_transforms), len(m.scene.tlas_nodes)), op
        if op[0] in ("tlas", "scene"):
            assert m.tlas_fresh
        if m.tlas_fresh:
            for builder in (native_builder, oracle_builder):
                c = copy.deepcopy(m.scene); S.rebuild_tlas(c, builder)
                assert c.tlas_nodes.tobytes() == m.scene.tlas_nodes.tobytes(), op
        if op[0] == "verts":
            moved = np.abs(m.scene.vertex_positions - pristine[m.name]).max()
            assert 0 < moved                                                               # (each verts op moves by at most 0.05; several may add up)
        keep = dict(m.settings); m.settings["RayDepth"] = 1
        o = m.oracle_frame(oracle_mod); img = o.image(0); o.close(); m.settings = keep
        assert np.isfinite(img).all() and img.shape == (U.H, U.W, 4), op
        hits = m.oracle_hits(oracle_mod, U.query_rays(5, n=64, short=8))
        assert len(hits) == 64
    for k, v in scenes.items():                                                             # the shared scenes stay what they were (the mirror works on copies)
        assert v.vertex_positions.tobytes() == pristine[k].tobytes()
