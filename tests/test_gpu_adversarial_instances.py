"""The device TLAS build (idkptBuildTlasOnDevice -> k_tlas_build, csrc/kernels_scene.hpp) on ADVERSARIAL instance sets (tests/adversarial_instances.py;
tests/test_adversarial_instances_ref.py proves on the CPU that the cases are what they claim): the node array of the oracle's serial build, byte for byte, at every radius of
every case and again after the transforms moved; and, for one small case per class, the frame traced through the device-built tree (UseTlas = 1) and the frame of the same
instance set through the instance loop / the library's own trees (UseTlas = 0) against the oracle.  There is no tolerance in this file."""
import copy
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import configs  # noqa: E402
import adversarial_instances as A  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import assert_equal, oracle_render  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = 64, 40


@pytest.fixture(scope="module")
def built(native_builder, oracle_builder):
    """per case: the scene (no TLAS in it), its moved twin, and the oracle's node arrays of both per radius — computed once, shared, never written to"""
    cache = {}

    def get(name):
        if name not in cache:
            case = A.CASES[name]
            sc = case.factory(native_builder)
            moved = copy.copy(sc); moved.mesh_transforms = A.permuted(sc)
            out = []
            for s in (sc, moved):
                bounds = A.bounds_of(s, oracle_builder)
                A.finite_union(bounds)
                out.append((s, bounds, {r: oracle_builder.build_tlas(bounds, r) for r in case.radii}))
            cache[name] = out
        return cache[name]
    return get


def _build_and_compare(pt, label, n, r, want):
    pt.BuildTlasOnDevice(r)
    got = pt.DownloadBuffer(T.IDKPT_BUF_TLAS_NODES, T.GpuTlasNode, 2 * n - 1)
    assert got.tobytes() == want.tobytes(), f"{label} radius {r}: {A.first_difference(got, want)}"


@pytest.mark.parametrize("cls", A.CLASSES)
def test_device_build_equals_the_oracle(built, cls):
    """one context per class; per case an upload, per radius a build and a download; then the transforms dealt anew among the instances (the tie structure survives) and
    every radius again"""
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(8, 8)
    try:
        for name in [k for k in A.CASES if A.CASES[k].cls == cls]:
            (sc, _, want), (moved, _, want_moved) = built(name)
            n = len(sc.blas_instances)
            pt.UploadScene(sc)
            for r in A.CASES[name].radii:
                _build_and_compare(pt, name, n, r, want[r])
            if n > 1:
                pt.UpdateBuffer(T.IDKPT_BUF_MESH_TRANSFORMS, moved.mesh_transforms)
                for r in A.CASES[name].radii:
                    _build_and_compare(pt, name + " (moved)", n, r, want_moved[r])
    finally:
        pt.Dispose()


@pytest.mark.parametrize("name", [k for k in A.CASES if A.CASES[k].render])
def test_frames_through_the_device_built_tree_and_through_the_loop(built, oracle_mod, name):
    """64 x 40, RayDepth 2, one sample, a camera that looks at the cluster.  UseTlas = 1: the GPU walks the tree it built itself, the oracle the oracle-built one.  UseTlas = 0:
    the instance loop — on the GPU whatever the host routes these layouts to (the loop, the library's own padded TLAS, the braid); mirrored, flat and zero-scale instances
    included, it must give the loop's frame."""
    from idkengine_amd.pathtracer import PathTracer
    (sc, bounds, want), _ = built(name)
    n = len(sc.blas_instances); assert n <= 64
    cam = A.camera_for(bounds, W, H)
    r = 15
    host = copy.copy(sc); host.tlas_nodes = want[r]
    for use_tlas in (1, 0):
        ov = dict(RayDepth=2, UseTlas=use_tlas)
        o = oracle_render(oracle_mod, host, cam, W, H, **ov)
        pt = PathTracer(W, H, settings=configs.apply_settings(T.Settings.default(), ov))
        try:
            pt.UploadScene(sc); pt.SetCamera(cam)                 # (no TLAS uploaded: the only tree the context can walk is the one it builds)
            pt.enable_counters(False); pt.enable_primary_hit_capture(True)
            _build_and_compare(pt, name, n, r, want[r])
            pt.Compute(); pt.flush()
            assert_equal(pt, o, counters=False)
            hits = int((o.primary_hits()[1] != 0xFFFFFFFF).sum())
            assert hits > 0, f"{name}: the camera sees nothing of the cluster"
            print(f"{name} UseTlas {use_tlas}: {hits} of {W * H} primary rays hit")
        finally:
            pt.Dispose(); o.close()


def test_radius_is_validated_and_the_context_goes_on(built):
    from idkengine_amd.pathtracer import PathTracer
    from idkengine_amd._lib import IdkPtError
    (sc, _, want), _ = built("radius_n40")
    pt = PathTracer(8, 8)
    try:
        pt.UploadScene(sc)
        for bad in (0, -1):
            with pytest.raises(IdkPtError):
                pt.BuildTlasOnDevice(bad)
        _build_and_compare(pt, "radius_n40 after refused radii", 40, 15, want[15])
    finally:
        pt.Dispose()
