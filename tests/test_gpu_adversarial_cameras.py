"""The first-hit stage on ADVERSARIAL cameras (tests/adversarial_cameras.py; tests/test_adversarial_cameras_ref.py proves on the CPU that the cases are what they claim).
Everything is compared on bytes; there is no tolerance in this file.
  1  soundness, read directly: the tile classes of a batch (idkptDownloadTileClasses) against the oracle's own primary rays and first box tests — a class 1-8 only where no
     ray of the tile can pass a first box test, a class 1-6 only where all of them see that one sky face, 7 / 8 only without / under a textured sky; all zeros (or no
     classification at all) behind every gate of the rule
  2  not vacuous: every tile the documented rule, restated in binary64 with doubled allowances, calls clearly empty carries a class
  3  end to end: the frames with the classification, with no_tile_cull = 1 and of the oracle agree on every bit — 16 samples per pixel, as 16 batches of 1 (the per-sample flag
     path), as one batch of 16 (pixel-major: the workgroup returns), as a frame ring of four cameras in one batch, and as two batches in a row
"""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import configs  # noqa: E402
import adversarial_cameras as A  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import assert_equal, bits  # noqa: E402

pytestmark = pytest.mark.gpu
SPP = 16


@pytest.fixture(scope="module")
def scenes(native_builder):
    cache = {}

    def get(case):
        k = case.scene_key()
        if k not in cache:
            cache[k] = A.make_scene(case.scene, native_builder, sky=case.sky, **case.scene_kw)
        return cache[k]
    return get


@pytest.fixture(scope="module")
def truths(oracle_mod, scenes):
    """the oracle's truth per (case, UseTlas, member): computed once, shared by the tests"""
    cache = {}

    def get(case, use_tlas, member=0, own_tree=False):
        k = (case.name, use_tlas, member)
        rows = A.local_rows(case, member)
        if k not in cache:
            cache[k] = A.truth(oracle_mod, case, scenes(case), use_tlas, rows)
        if k + (own_tree,) not in cache:
            cache[k + (own_tree,)] = A.clearly_empty(case, scenes(case), use_tlas, rows, own_tree=own_tree)
        return cache[k], cache[k + (own_tree,)]
    return get


def _pt(case, sc, plan, member=None, group=False, **ov):
    """a context of the case under a walk plan: the whole frame, the case's group of members on one device (group), one member of it alone (member), or its strip"""
    from idkengine_amd.pathtracer import PathTracer
    options, use_tlas = A.PLANS[plan]
    w, h = case.frame
    st = configs.apply_settings(T.Settings.default(), case.settings(UseTlas=use_tlas, **ov))
    kind = case.rows[0] if case.rows else None
    if kind == "members" and group:
        pt = PathTracer(w, h, settings=st, devices=[0] * case.rows[1])
    elif kind == "members":
        pt = PathTracer(w, h, settings=st, row_modulo=case.rows[1], row_remainder=member or 0, row_band=8)
    else:
        pt = PathTracer(w, h, settings=st)
        if kind == "range":
            pt.SetRowRange(case.rows[1], case.rows[2])
    for k, v in options.items():
        pt.set_option(k, v)
    pt.UploadScene(sc); pt.SetPerFrameData(case.pf)
    return pt


def _oracle(O, case, sc, plan, member=None, **ov):
    kind = case.rows[0] if case.rows else None
    w, h = case.frame
    if kind == "members" and member is not None:
        o = O.OraclePathTracer(sc, w, h, row_modulo=case.rows[1], row_remainder=member, row_band=8)
    else:
        o = O.OraclePathTracer(sc, w, h)
        if kind == "range":
            o.set_row_range(case.rows[1], case.rows[2])
    o.set_perframe_data(case.pf)
    configs.apply_settings(o.settings, case.settings(UseTlas=A.PLANS[plan][1], **ov)); o.enable_counters(True)
    return o


def check_classes(label, case, sc, cls, tr, ce, expect=None):
    """cls: (tilesY, tilesX) classes of one set; tr / ce: the truth and the clearly empty tiles of the same context"""
    expect = expect or case.expect
    assert cls.shape == tr.can_hit.shape, f"{label}: {cls.shape} classes for {tr.can_hit.shape} tiles"
    sky_n = 0 if sc.sky_faces is None else sc.sky_faces.shape[1]
    if expect == "zero":
        assert not cls.any(), f"{label}: tiles {np.argwhere(cls != 0)[:4].tolist()} carry classes {cls[cls != 0][:4].tolist()} behind a shut gate"
        return
    for ty, tx in np.argwhere(cls != 0):
        c = int(cls[ty, tx])
        assert 1 <= c <= 8, f"{label}: tile ({tx}, {ty}) has class {c}"
        assert not tr.can_hit[ty, tx], f"{label}: tile ({tx}, {ty}) has class {c}, but the ray of {A.describe_ray(tr.first[ty, tx])} passes a first box test"
        if c <= 6:
            assert sky_n == 1 and int(tr.faces[ty, tx]) == 1 << (c - 1), f"{label}: tile ({tx}, {ty}) has class {c} (sky face {c - 1}), its rays see the faces {[f for f in range(6) if tr.faces[ty, tx] >> f & 1]} of a sky of size {sky_n}"
        else:
            assert (c == 7) == (sky_n == 0) and (c == 8) == (sky_n > 1), f"{label}: tile ({tx}, {ty}) has class {c} under a sky of size {sky_n}"
    missed = np.argwhere(ce & (cls == 0))
    assert len(missed) == 0, f"{label}: the clearly empty tiles {missed[:6][:, ::-1].tolist()} (x, y) carry no class ({len(missed)} of {int(ce.sum())})"


@pytest.mark.parametrize("name", list(A.CASES))
def test_tile_classes_are_sound_and_not_vacuous(scenes, truths, name):
    case = A.CASES[name]; sc = scenes(case)
    members = range(case.rows[1]) if case.rows and case.rows[0] == "members" else (None,)
    for plan in A.plans_of(case):
        for member in members:
            pt = _pt(case, sc, plan, member=member)
            try:
                pt.Compute(); pt.flush()
                cls = pt.tile_classes()
            finally:
                pt.Dispose()
            label = f"{name} plan {plan}" + ("" if member is None else f" member {member}")
            if case.expect == "none":
                assert cls.shape[0] == 0, f"{label}: {cls.shape[0]} sets of classes where nothing is classified"
                continue
            assert cls.shape[0] == 1, f"{label}: {cls.shape[0]} sets"
            tr, ce = truths(case, A.PLANS[plan][1], member or 0, own_tree=plan in A.OWN_TREE_PLANS)
            check_classes(label, case, sc, cls[0], tr, ce)
            print(f"{label}: {int((cls[0] != 0).sum())} of {cls[0].size} tiles classified, {int(ce.sum())} clearly empty, {int(tr.can_hit.sum())} can hit")


def test_a_group_reports_member_0(scenes, truths):
    """idkptDownloadTileClasses on a multi-device context: the tiles of member 0"""
    case = A.CASES["bands_75x37_2_members"]; sc = scenes(case)
    pt = _pt(case, sc, "one_blas", group=True)
    try:
        pt.Compute(); pt.flush()
        cls = pt.tile_classes()
    finally:
        pt.Dispose()
    tr, ce = truths(case, 0, 0)
    assert cls.shape[0] == 1
    check_classes("group of 2", case, sc, cls[0], tr, ce)


def _state(pt):
    st = pt.stats()
    return {"image": pt.Result.copy(), "rays": pt.rays().tobytes(), "alive": pt.alive_queue().copy(), "alive_counts": st["alive_counts"][1:], "rays_traced": st["rays_traced"],
            "hits": [a.copy() for a in pt.primary_hits()], "visits": (st["node_pair_visits"], st["triangle_tests"])}


def _same(label, a, b, visits):
    assert (bits(a["image"]) == bits(b["image"])).all(), f"{label}: images differ at pixels {np.argwhere((bits(a['image']) != bits(b['image'])).any(-1))[:4].tolist()}"
    assert a["rays"] == b["rays"], f"{label}: ray records differ"
    assert (a["alive"] == b["alive"]).all() and a["alive_counts"] == b["alive_counts"] and a["rays_traced"] == b["rays_traced"], f"{label}: queues / counts differ"
    for x, y in zip(a["hits"], b["hits"]):
        assert (bits(x) == bits(y)).all(), f"{label}: primary hits differ"
    if visits:
        assert a["visits"] == b["visits"], f"{label}: visit counters differ: {a['visits']} / {b['visits']}"


def _e2e_plans(case):
    return A.plans_of(case) if case.name in ("inst", "same_space", "silhouette_exact") else A.plans_of(case)[:1]


@pytest.mark.parametrize("batch", [1, SPP], ids=["batches_of_1", "one_batch_of_16"])
@pytest.mark.parametrize("name", list(A.CASES))
def test_frames_equal_the_oracle_with_and_without_the_classification(oracle_mod, scenes, name, batch):
    """16 samples per pixel (the jitters reach the sliver), RayDepth 2: the GPU with the classification == the GPU with no_tile_cull = 1 == the oracle — image, ray records
    (k_regen_culled), alive queue, alive_counts, rays_traced, primary hits (k_fill_miss), and the visit counters of the counting build under the walks that reproduce them.
    A group of members is also held to the oracle's whole frame — and with it to the one-device context."""
    case = A.CASES[name]; sc = scenes(case)
    group = bool(case.rows) and case.rows[0] == "members"
    for plan in _e2e_plans(case):
        counting = plan in A.COUNTING_PLANS and not group
        o = _oracle(oracle_mod, case, sc, plan, SamplesPerPixel=SPP); o.render()
        got = {}
        for cull_off in (0, 1):
            pt = _pt(case, sc, plan, group=group, SamplesPerPixel=SPP)
            try:
                pt.set_option("no_tile_cull", cull_off)
                pt.enable_counters(counting); pt.enable_primary_hit_capture(True); pt.set_max_batch(batch)
                pt.Compute(); pt.flush()
                assert_equal(pt, o, counters=counting)
                got[cull_off] = _state(pt)
                if not group:
                    sets = pt.tile_classes().shape[0]
                    assert sets == (0 if cull_off or case.expect == "none" else 1), f"{name} {plan}: {sets} sets with no_tile_cull = {cull_off}"
            finally:
                pt.Dispose()
        o.close()
        _same(f"{name} plan {plan} batch {batch}", got[0], got[1], counting)
        if case.rows:
            # ... and directly to ONE device that holds the whole frame: the group's frame is that frame, the strip's rows are its rows
            whole = A.Case(case.name, case.cls, scene=case.scene, frame=case.frame, pf=case.pf, focal=case.focal, radius=case.radius, sky=case.sky, scene_kw=case.scene_kw)
            pt = _pt(whole, sc, plan, SamplesPerPixel=SPP)
            try:
                pt.set_max_batch(batch); pt.Compute(); pt.flush()
                img = pt.Result.copy()
            finally:
                pt.Dispose()
            rows = slice(None) if group else A.local_rows(case)
            assert (bits(got[0]["image"]) == bits(img[rows])).all(), f"{name} plan {plan} batch {batch}: differs from the one-device context"


RING = ("silhouette_exact", "apex_straddling", "fov_off_diagonal", "near_2p-10")     # four cameras on the same scene and settings


def test_a_frame_ring_of_four_cameras_in_one_batch(oracle_mod, scenes, truths):
    """tilePerSample: one classification per sample of the batch, each with the camera of its frame: 16 sets, every one held to the truth of its camera; the four frames == the oracle's"""
    cases = [A.CASES[n] for n in RING]; sc = scenes(cases[0])
    assert len({c.scene_key() for c in cases}) == 1 and len({(c.focal, c.radius, c.frame) for c in cases}) == 1
    per = SPP // 4
    frames = {}
    for cull_off in (0, 1):
        pt = _pt(cases[0], sc, "one_blas", SamplesPerPixel=per)
        try:
            pt.set_option("no_tile_cull", cull_off); pt.SetFrameRing(4); pt.set_max_batch(SPP)
            slots = []
            for c in cases:
                slots.append(pt.BeginFrame()); pt.SetPerFrameData(c.pf); pt.Compute()
            pt.flush()
            cls = pt.tile_classes()
            frames[cull_off] = [pt.FrameResult(s).copy() for s in slots] + [np.frombuffer(pt.rays().tobytes(), np.uint8)]
        finally:
            pt.Dispose()
        if cull_off:
            assert cls.shape[0] == 0
            continue
        assert cls.shape[0] == SPP, f"{cls.shape[0]} sets for a batch of {SPP} samples with their own cameras"
        for k in range(SPP):
            tr, ce = truths(cases[k // per], 0)
            check_classes(f"ring sample {k} ({RING[k // per]})", cases[k // per], sc, cls[k], tr, ce)
    for f, c in enumerate(cases):
        o = _oracle(oracle_mod, c, sc, "one_blas", SamplesPerPixel=per); o.render()
        for cull_off in (0, 1):
            assert (bits(frames[cull_off][f]) == bits(o.image(0))).all(), f"frame {f} ({c.name}) no_tile_cull {cull_off}"
        if f == 3:
            assert frames[0][4].tobytes() == o.rays().tobytes() == frames[1][4].tobytes()
        o.close()


def test_two_batches_in_a_row_with_different_tile_sets(oracle_mod, scenes, truths):
    """the second camera classifies other tiles than the first: nothing of the first batch's classes, flag bytes or ray state may show in the second"""
    a, b = A.CASES["apex_behind_off_axis"], A.CASES["silhouette_exact"]; sc = scenes(a)
    assert a.scene_key() == b.scene_key()
    for batch in (1, SPP):
        pt = _pt(a, sc, "one_blas", SamplesPerPixel=SPP)
        try:
            pt.enable_counters(True); pt.enable_primary_hit_capture(True); pt.set_max_batch(batch)
            pt.Compute(); pt.flush()
            first = pt.tile_classes()[0].copy()
            pt.SetPerFrameData(b.pf); pt.ResetAccumulation(); pt.reset_stats()
            pt.Compute(); pt.flush()
            second = pt.tile_classes()[0].copy()
            assert (first != second).any()
            tr, ce = truths(b, 0)
            check_classes(f"second batch (batch {batch})", b, sc, second, tr, ce)
            o = _oracle(oracle_mod, b, sc, "one_blas", SamplesPerPixel=SPP); o.render()
            assert_equal(pt, o, counters=True)
            o.close()
        finally:
            pt.Dispose()
