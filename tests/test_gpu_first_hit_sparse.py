"""The first-hit stage on sparse views: pixel-major batches (8 samples or more under one camera and one scene version) store nothing for a tile k_classify_tiles proves to be
sky — its k_gen_primary workgroup returns at once, k_regen_culled takes "culled per tile" from the tile class, and the per-ray flag bytes keep the invariant "bit 0 is clear
between batches" (k_scan_local<true> clears what it consumes), so a byte an earlier batch left in such a tile cannot enqueue a ray.  Everything observable must be what it
was: the image, the downloaded ray state (k_regen_culled, finish_deferred), the alive queue, the counts and the ray statistics — against the CPU oracle and against the same
run with option no_tile_cull = 1, bit for bit.  The frame is 72 x 40 (five tile rows of 8, 72 is no multiple of 64: a 64-slot wave of the scan straddles rows); 72 x 40 is a
multiple of 64, so the resize case adds 75 x 37: padding slots, a partial tile column and a partial tile row."""
import copy
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

W, H = 72, 40
N_TRIS = 2000


def cam_a(w=W, h=H):
    return S.Camera(w, h, position=(0.0, 0.0, 7.0))                                  # the soup ([-2, 2]^3) in the middle of the frame: a few tiles traverse, the rest is sky


def cam_b(w=W, h=H):
    return S.Camera(w, h, position=(0.0, 0.0, 7.0), view_dir=(1.4, 0.1, -1.0))       # the soup near the left edge: the middle tiles are sky now


def cam_far(w=W, h=H):
    return S.Camera(w, h, position=(0.0, 0.0, 7.0), view_dir=(0.0, 0.0, 1.0))        # looking away: every tile is sky


def cam_inside(w=W, h=H):
    return S.Camera(w, h, position=(0.0, 0.0, 0.0))                                  # inside the soup: no tile is sky


@pytest.fixture(scope="module")
def soup(native_builder):
    return S.soup_scene(N_TRIS, native_builder, seed=3, extent=2.0, edge=0.6)


def textured_sky(seed=5, size=4):
    rng = np.random.default_rng(seed)
    f = np.ones((6, size, size, 4), np.float32); f[..., :3] = rng.uniform(0.0, 2.0, (6, size, size, 3)).astype(np.float32)
    return f


def with_sky(sc, faces):
    out = copy.copy(sc)
    out.sky_faces = np.ascontiguousarray(faces, np.float32)
    return out


def new_pt(sc, w=W, h=H, max_batch=32, no_tile_cull=0, defer_last=1, devices=None, **ov):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h, settings=configs.apply_settings(T.Settings.default(), ov), devices=devices)
    pt.set_option("no_tile_cull", no_tile_cull); pt.set_option("defer_last", defer_last)
    pt.UploadScene(sc); pt.set_max_batch(max_batch)
    return pt


def new_oracle(O, sc, cam, w=W, h=H, **ov):
    o = O.OraclePathTracer(sc, w, h); o.set_camera(cam); configs.apply_settings(o.settings, ov)
    return o


def state(pt):
    """Everything a caller can see of the last launched batch.  The downloads come after the image: they complete what the batch deferred."""
    img = pt.Result.copy(); st = pt.stats()
    rays = pt.rays().copy(); q = pt.alive_queue().copy()
    return {"image": img, "rays": rays, "queue": q, "image_after": pt.Result.copy(), "rays_traced": pt.stats()["rays_traced"], "rays_traced_before": st["rays_traced"], "alive_counts": list(pt.stats()["alive_counts"])}


def assert_same_state(a, b, depth, what):
    assert (bits(a["image"]) == bits(b["image"])).all(), what
    assert (bits(a["image_after"]) == bits(b["image_after"])).all(), what
    assert a["rays"].tobytes() == b["rays"].tobytes(), what
    assert a["queue"].shape == b["queue"].shape and (a["queue"] == b["queue"]).all(), what
    assert a["rays_traced"] == b["rays_traced"] and a["rays_traced_before"] == b["rays_traced_before"], what
    assert a["alive_counts"][:depth + 1] == b["alive_counts"][:depth + 1], what


def assert_equals_oracle(s, o, what):
    assert (bits(s["image"]) == bits(o.image(0))).all(), what
    assert (bits(s["image_after"]) == bits(o.image(0))).all(), what
    assert s["rays"].tobytes() == o.rays().tobytes(), what
    oq = o.alive_queue()
    assert s["queue"].shape == oq.shape and (s["queue"] == oq).all(), what


def batch(pt, cam, B, reset=True):
    if reset:
        pt.ResetAccumulation()
    pt.SetCamera(cam)
    for _ in range(B):
        pt.Compute()
    return state(pt)


def oracle_batch(O, sc, cam, B, w=W, h=H, **ov):
    o = new_oracle(O, sc, cam, w, h, **ov)
    for _ in range(B):
        o.render()
    return o


@pytest.mark.parametrize("defer_last", [0, 1])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("B", [1, 7, 8, 20, 32])
def test_batches_on_a_sparse_view(soup, oracle_mod, B, depth, defer_last):
    """Batches below and above the pixel-major threshold (8), sizes that do and do not divide into equal groups of at most 16 samples; two batches in a row on one context
    (the second one meets the bytes of the first), then a third of another size (the count mirrors of the previous batch do not fit)."""
    pt = new_pt(soup, defer_last=defer_last, RayDepth=depth); twin = new_pt(soup, no_tile_cull=1, defer_last=defer_last, RayDepth=depth)
    o = new_oracle(oracle_mod, soup, cam_a(), RayDepth=depth)
    rays_expected = 0
    for k, n in enumerate((B, B, 9 if B != 9 else 8)):
        a = batch(pt, cam_a(), n, reset=False); b = batch(twin, cam_a(), n, reset=False)
        for _ in range(n):
            o.render()
        assert_same_state(a, b, depth, (k, n)); assert_equals_oracle(a, o, (k, n))
        assert a["rays_traced"] == o.stats()["rays_traced"], (k, n)
        rays_expected = a["rays_traced"]
    # the view is what the case claims: most primary rays never enter the traversal, some do, and some of those continue
    assert 0 < a["alive_counts"][0] < 9 * W * H // 2 and len(a["queue"]) > 0 and rays_expected > 0
    pt.Dispose(); twin.Dispose(); o.close()


@pytest.mark.parametrize("sizes", [(32, 32, 32), (32, 8, 20)])
@pytest.mark.parametrize("sky_change", [False, True])
def test_stale_flags_of_a_tile_that_becomes_sky(soup, oracle_mod, sizes, sky_change):
    """Camera A: the middle tiles traverse and some of their rays continue (flag bit 0 set during the batch).  Camera B: the same tiles are sky, and nothing is written for
    them.  Then A again.  No reallocation in between (the batch size changes by flushing early, not by idkptSetMaxBatch); with sky_change the sky goes constant -> textured
    (tile class 8) -> constant between the batches.  Every batch is downloaded, and equals a context that never saw another camera or sky."""
    depth = 3
    pt = new_pt(soup, RayDepth=depth); twin = new_pt(soup, no_tile_cull=1, RayDepth=depth)
    tex = textured_sky(); plain = soup.sky_faces
    steps = [(cam_a(), plain), (cam_b(), tex if sky_change else plain), (cam_a(), plain), (cam_b(), plain)]
    mid = (H // 2) * W + W // 2                      # a pixel of the middle tile
    for k, (cam, sky) in enumerate(steps):
        n = sizes[k % len(sizes)]
        if sky_change:
            for p in (pt, twin):
                p.UpdateSky(sky)
        sc = with_sky(soup, sky)
        a = batch(pt, cam, n); b = batch(twin, cam, n)
        o = oracle_batch(oracle_mod, sc, cam, n, RayDepth=depth)
        assert_same_state(a, b, depth, k); assert_equals_oracle(a, o, k)
        hit_mid = np.isfinite(o.primary_hits()[0][mid]) and o.primary_hits()[0][mid] < 1e30
        assert hit_mid == (k % 2 == 0), k           # A: the middle pixel hits the soup; B: it is sky
        o.close()
    pt.Dispose(); twin.Dispose()


def test_frame_ring_and_scene_versions_in_one_batch(native_builder, oracle_mod):
    """Four cameras and two states of the geometry in one batch (one classification per sample: the path that still writes a byte per classified pixel), after a
    pixel-major batch left its bytes behind.  Against the same run without the tile classes, against every frame rendered alone, and — for the frames of the
    unmodified geometry — against the oracle."""
    sc = S.soup_scene(N_TRIS, native_builder, seed=3, extent=2.0, edge=0.6, refittable=True)
    moved = (sc.vertex_positions + np.float32(0.2) * np.sin(sc.vertex_positions[:, ::-1] * 1.7).astype(np.float32)).astype(np.float32)
    cams = [cam_a(), cam_b(), cam_a(), cam_b()]
    out = {}
    for name, cull_off, versions, mb in (("batched", 0, 2, 4), ("batched_no_tile_cull", 1, 2, 4), ("alone", 0, 1, 1)):
        pt = new_pt(sc, max_batch=32, no_tile_cull=cull_off, RayDepth=3)
        batch(pt, cam_a(), 16)                                            # pixel-major: leaves the bytes of the sky tiles as they were
        pt.SetSceneVersions(versions); pt.SetFrameRing(4); pt.set_max_batch(mb)
        slots = []
        for f in range(4):
            if f == 2:
                pt.UpdateBuffer(T.IDKPT_BUF_VERTEX_POSITIONS, moved); pt.RefitBlas(0)
            slots.append(pt.BeginFrame()); pt.SetCamera(cams[f]); pt.Compute()
        frames = [pt.FrameResult(s).copy() for s in slots]
        out[name] = (frames, pt.rays().copy(), pt.alive_queue().copy(), pt.stats()["rays_traced"])
        pt.Dispose()
    for name in ("batched_no_tile_cull", "alone"):
        for f in range(4):
            assert (bits(out["batched"][0][f]) == bits(out[name][0][f])).all(), (name, f)
        assert out["batched"][1].tobytes() == out[name][1].tobytes(), name
        assert (out["batched"][2] == out[name][2]).all() and out["batched"][3] == out[name][3], name
    for f in range(2):
        o = oracle_batch(oracle_mod, sc, cams[f], 1, RayDepth=3)
        assert (bits(out["batched"][0][f]) == bits(o.image(0))).all(), f
        o.close()


def test_light_hits_switch_the_pre_cull_off(native_builder, oracle_mod):
    """DoTraceLights with one light: no pre-cull and no tile classes (every ray traverses), on a context whose previous batch had them."""
    sc = S.soup_scene(N_TRIS, native_builder, seed=3, extent=2.0, edge=0.6)
    sc.lights = S.make_lights([((0.0, 1.0, 4.0), 0.5, (20.0, 20.0, 20.0))])
    depth = 3
    pt = new_pt(sc, RayDepth=depth); twin = new_pt(sc, no_tile_cull=1, RayDepth=depth)
    for lights, n in ((0, 16), (1, 8), (0, 16), (1, 3)):
        for p in (pt, twin):
            p.DoTraceLights = lights
        a = batch(pt, cam_a(), n); b = batch(twin, cam_a(), n)
        o = oracle_batch(oracle_mod, sc, cam_a(), n, RayDepth=depth, DoTraceLights=lights)
        assert_same_state(a, b, depth, (lights, n)); assert_equals_oracle(a, o, (lights, n))
        o.close()
    pt.Dispose(); twin.Dispose()


def test_resize_between_batches(soup, oracle_mod):
    """idkptSetSize to a smaller and then a larger frame (75 x 37: padding slots, a partial tile column and a partial tile row), batches on both sides of the threshold."""
    depth = 3
    pt = new_pt(soup, RayDepth=depth); twin = new_pt(soup, no_tile_cull=1, RayDepth=depth)
    for (w, h), n in (((W, H), 16), ((40, 24), 16), ((75, 37), 20), ((75, 37), 5), ((75, 37), 32)):
        for p in (pt, twin):
            if (p.width, p.rows) != (w, h):
                p.SetSize(w, h)
        cam = cam_a(w, h)
        a = batch(pt, cam, n); b = batch(twin, cam, n)
        o = oracle_batch(oracle_mod, soup, cam, n, w, h, RayDepth=depth)
        assert_same_state(a, b, depth, (w, h, n)); assert_equals_oracle(a, o, (w, h, n))
        o.close()
    pt.Dispose(); twin.Dispose()


@pytest.mark.parametrize("view", ["none_classified", "all_classified"])
def test_views_without_and_with_only_sky_tiles(soup, oracle_mod, view):
    depth = 3
    cam = cam_inside() if view == "none_classified" else cam_far()
    pt = new_pt(soup, RayDepth=depth); twin = new_pt(soup, no_tile_cull=1, RayDepth=depth)
    batch(pt, cam_a(), 16); batch(twin, cam_a(), 16)                      # bytes of another view first
    for n in (16, 32, 4):
        a = batch(pt, cam, n); b = batch(twin, cam, n)
        o = oracle_batch(oracle_mod, soup, cam, n, RayDepth=depth)
        assert_same_state(a, b, depth, n); assert_equals_oracle(a, o, n)
        if view == "all_classified":
            assert a["alive_counts"][0] == 0 and len(a["queue"]) == 0
        else:
            assert a["alive_counts"][0] > n * W * H // 2
        o.close()
    pt.Dispose(); twin.Dispose()


def test_two_members_with_bands_of_8_rows(soup):
    """ONE context on two members that share the device (bands of 8 rows): pixel-major batches on row-sharded frames, against the one-device context."""
    import ctypes as C
    from idkengine_amd import _lib
    n = C.c_int32(0); _lib.load().idkptGetDeviceCount(C.byref(n))
    ids = [i % max(1, n.value) for i in range(2)]
    for depth in (2, 3):
        grp = new_pt(soup, devices=ids, RayDepth=depth); grp.SetGroupSharding(3); one = new_pt(soup, RayDepth=depth)
        for cam, nb in ((cam_a(), 16), (cam_b(), 32), (cam_a(), 8), (cam_a(), 3)):
            outs = []
            for p in (grp, one):
                p.ResetAccumulation(); p.SetCamera(cam)
                for _ in range(nb):
                    p.Compute()
                outs.append((p.Result.copy(), p.stats()["rays_traced"], p.rays().copy() if depth > 2 else None, p.alive_queue().copy() if depth > 2 else None))
            assert (bits(outs[0][0]) == bits(outs[1][0])).all() and outs[0][1] == outs[1][1], (depth, nb)
            if depth > 2:                                                 # (RayDepth 2 on interleaved bands: the state the last bounce leaves is slot-seeded, tests/test_gpu_multi.py)
                assert outs[0][2].tobytes() == outs[1][2].tobytes() and (outs[0][3] == outs[1][3]).all(), (depth, nb)
        grp.Dispose(); one.Dispose()
