"""idkptSkin (k_skin) and the refit behind it (k_refit_leaves / k_refit_level) on the adversarial skeletons of tests/adversarial_skeletons.py: positions, PREVIOUS positions
and the re-compressed vertices equal tests/skin_ref.py byte for byte (NaN positions by class), the refitted nodes equal oracle_builder.refit on the restatement's positions,
every `refused` case is refused before anything is launched, and frames equal the oracle rendering a host scene in which NOTHING was downloaded from the device.

Every case is run — none is skipped or filtered by what the device returns.  Non-finite positions into the refit are out of scope (tests/adversarial_skeletons.py says
why): the RESTATEMENT decides which cases have finite skinned positions, and exactly those are refitted."""
import copy
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import configs  # noqa: E402,F401
from idkengine_amd import scenes as S, gputypes as T  # noqa: E402
from idkengine_amd._lib import IdkPtError  # noqa: E402
from gpu_helpers import bits, oracle_render  # noqa: E402
import skin_ref as R  # noqa: E402
import adversarial_skeletons as A  # noqa: E402

pytestmark = pytest.mark.gpu
LAUNCHED = [c for c in A.CASES if not c["refused"]]
REFUSED = [c for c in A.CASES if c["refused"]]
assert len(LAUNCHED) + len(REFUSED) == len(A.CASES) and len(REFUSED) >= 6


def _poisoned(sc, case):
    """the scene's positions and vertices with everything OUTSIDE the case's output range replaced by marks (finite: the refit reads them): a write past the range shows"""
    _, o, _, n = case["args"]
    nv = len(sc.vertices)
    outside = np.ones(nv, bool); outside[o:min(o + n, nv)] = False
    pos = sc.vertex_positions.reshape(-1, 3).copy(); verts = sc.vertices.copy()
    k = np.arange(nv, dtype=np.float32)
    pos[outside] = np.stack([1000.0 + k, -2000.0 - k, 3000.0 + 0.5 * k], 1)[outside]
    verts["Normal"][outside] = (0xDEAD0000 + np.arange(nv, dtype=np.uint32))[outside]; verts["Tangent"][outside] = (0xBEEF0000 + np.arange(nv, dtype=np.uint32))[outside]
    verts["TexCoord"] = np.stack([k + 0.25, -k - 0.75], 1)                      # uv words everywhere, inside the range too: they are copied, never computed
    return pos, verts


def _context(case, sc, devices=None, poison=True, size=(8, 8)):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(size[0], size[1], devices=devices); pt.UploadScene(sc)
    pos, verts = _poisoned(sc, case) if poison else (sc.vertex_positions.reshape(-1, 3).copy(), sc.vertices.copy())
    if poison:
        pt.UpdateBuffer(T.IDKPT_BUF_VERTEX_POSITIONS, pos); pt.UpdateBuffer(T.IDKPT_BUF_VERTICES, verts)
    pt.UploadUnskinnedVertices(case["un"]); pt.UpdateBuffer(T.IDKPT_BUF_JOINT_MATRICES, case["joints"])
    return pt, pos, verts


def _download(pt, nv):
    return (pt.DownloadBuffer(T.IDKPT_BUF_VERTEX_POSITIONS, np.float32, 3 * nv).reshape(nv, 3), pt.DownloadBuffer(T.IDKPT_BUF_PREV_VERTEX_POSITIONS, np.float32, 3 * nv).reshape(nv, 3),
            pt.DownloadBuffer(T.IDKPT_BUF_VERTICES, T.GpuVertex, nv))


def _assert_state(got, want, where):
    assert R.same_positions(got[0], want[0]), (where, "positions")
    assert R.same_positions(got[1], want[1]), (where, "previous positions")
    assert R.same_vertices(got[2], want[2]), (where, "vertices")


def _blas1(sc):
    d = sc.blas_descs[1]
    return slice(d["NodeOffset"], d["NodeOffset"] + d["NodeCount"]), slice(d["TriangleOffset"], d["TriangleOffset"] + d["TriangleCount"])


def _refit_want(sc, pos, oracle_builder):
    ns, ts = _blas1(sc)
    nodes = sc.blas_nodes.copy()
    nodes[ns] = oracle_builder.refit(sc.blas_nodes[ns], np.ascontiguousarray(pos, np.float32), sc.blas_triangles[ts])
    return nodes


@pytest.mark.parametrize("case", LAUNCHED, ids=[c["name"] for c in LAUNCHED])
def test_skin_equals_the_restatement_and_the_refit_the_oracle(case, native_builder, oracle_builder):
    sc = A.scene(case, native_builder); nv = len(sc.vertices)
    pt, pos, verts = _context(case, sc)
    want = R.skin(case["un"], case["joints"], pos, verts, *case["args"])
    pt.Skin(*case["args"]); pt.synchronize()
    _assert_state(_download(pt, nv), want, case["name"])
    if case["joints2"] is not None:                                              # the same range again with other joints: prev must hold the FIRST call's positions
        pt.UpdateBuffer(T.IDKPT_BUF_JOINT_MATRICES, case["joints2"]); pt.Skin(*case["args"]); pt.synchronize()
        first = want
        want = R.skin(case["un"], case["joints2"], first[0], first[2], *case["args"], prev_positions=first[1])
        o, n = case["args"][1], case["args"][3]
        assert want[1][o:o + n].tobytes() == first[0][o:o + n].tobytes()
        _assert_state(_download(pt, nv), want, case["name"] + " (second call)")
    if np.isfinite(want[0]).all():                                               # chosen by the restatement, not by the device
        pt.RefitBlas(1); pt.synchronize()
        got = pt.DownloadBuffer(T.IDKPT_BUF_BLAS_NODES, T.GpuBlasNode, len(sc.blas_nodes))
        assert got.tobytes() == _refit_want(sc, want[0], oracle_builder).tobytes(), case["name"]
    else:
        assert case["cls"] in ("weights", "joints")
    pt.Dispose()


def test_every_finite_case_was_refitted():
    """the share of cases left out of the skin comparison is 0; of the refit, exactly the cases whose restated positions are not finite"""
    named = {"w_one_hot_inf_unused", "w_nan", "j_nan_entry", "j_inf_entry"}
    assert {c["name"] for c in LAUNCHED if "nan_position" in c["tags"]} == named
    assert sum(c["cls"] == "refit" for c in LAUNCHED) == 7 and not any("nan_position" in c["tags"] for c in LAUNCHED if c["cls"] == "refit")


@pytest.mark.parametrize("case", REFUSED, ids=[c["name"] for c in REFUSED])
def test_refused_cases_are_refused_before_any_launch(case, native_builder):
    from idkengine_amd import _lib
    assert _lib.load().idkptGetAbiVersion() >= 13, "a library without the joint-table check would launch the kernel on these: never send them to it"
    sc = A.scene(case, native_builder); nv = len(sc.vertices)
    pt, pos, verts = _context(case, sc)
    valid = (0, A.PAD, 0, 8)
    assert R.refusal(case["un"], len(case["joints"]), nv, *valid) is None and R.refusal(case["un"], len(case["joints"]), nv, *case["args"]) == case["refused"]
    want = R.skin(case["un"], case["joints"], pos, verts, *valid)
    pt.Skin(*valid); pt.synchronize()
    before = _download(pt, nv)
    _assert_state(before, want, "valid call before")
    with pytest.raises(IdkPtError) as e:
        pt.Skin(*case["args"])
    assert ("joint" if case["refused"] == "joint" else "range") in str(e.value), str(e.value)
    pt.synchronize()
    after = _download(pt, nv)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), "a refused call changes nothing"
    again = (8, A.PAD + 8, 0, 8)
    assert R.refusal(case["un"], len(case["joints"]), nv, *again) is None
    want = R.skin(case["un"], case["joints"], want[0], want[2], *again, prev_positions=want[1])
    pt.Skin(*again); pt.synchronize()
    _assert_state(_download(pt, nv), want, "valid call after")
    pt.Dispose()


def test_partial_range_into_another_scene_version(native_builder):
    """SetSceneVersions(2) with a queued sample pinning the current vertex state: the skin writes ANOTHER slot than it reads (verticesIn != vertices).  The uv words of the
    range and every word of the vertices outside it must arrive in the new state."""
    case = A.BY_NAME["r_input_is_not_output"]
    sc = A.scene(case, native_builder); nv = len(sc.vertices)
    pt, pos, verts = _context(case, sc, size=(16, 16))
    pt.SetSceneVersions(2); pt.SetFrameRing(2); pt.set_max_batch(2)
    pt.SetCamera(S.Camera(16, 16, position=(0.0, 0.5, 9.0), fovy_deg=60.0)); pt.RayDepth = 2
    pt.BeginFrame(); pt.Compute()                                                # queued, not launched: it reads the state the skin must not overwrite
    want = R.skin(case["un"], case["joints"], pos, verts, *case["args"])
    pt.Skin(*case["args"])
    pt.UpdateBuffer(T.IDKPT_BUF_JOINT_MATRICES, A.generic_joints()[::-1].copy())
    second = (0, A.PAD + 40, 0, 20)                                              # and a second partial range on top, back into the first slot or a fresh one
    want = R.skin(case["un"], A.generic_joints()[::-1].copy(), want[0], want[2], *second, prev_positions=want[1])
    pt.BeginFrame(); pt.Compute(); pt.Skin(*second); pt.synchronize()
    _assert_state(_download(pt, nv), want, "versions")
    pt.Dispose()


def test_whole_table_into_another_scene_version_reads_the_current_uv_words(native_builder):
    """A skin of the WHOLE vertex table goes to a free slot without a copy of the old state (verticesIn != vertices): the uv words must come from the CURRENT state (C), not from
    whatever the written slot held (the scene's own vertices, A).  Three versions; queued samples pin the states in turn."""
    case = A.BY_NAME["r_whole_table"]
    sc = A.scene(case, native_builder); nv = len(sc.vertices)
    pt, pos, verts = _context(case, sc, poison=False, size=(16, 16))
    pt.SetSceneVersions(3); pt.SetFrameRing(4); pt.set_max_batch(4)
    pt.SetCamera(S.Camera(16, 16, position=(0.0, 0.5, 9.0), fovy_deg=60.0)); pt.RayDepth = 2
    k = np.arange(nv, dtype=np.float32)
    b = verts.copy(); b["TexCoord"] = np.stack([k + 100.5, -k], 1); b["Normal"] ^= 1
    c = verts.copy(); c["TexCoord"] = np.stack([-k - 0.125, k + 7.0], 1); c["Tangent"] ^= 1
    pt.BeginFrame(); pt.Compute()                                                # pins state A
    pt.UpdateBuffer(T.IDKPT_BUF_VERTICES, b)
    pt.BeginFrame(); pt.Compute()                                                # pins state B
    pt.UpdateBuffer(T.IDKPT_BUF_VERTICES, c)
    pt.flush(); pt.synchronize()
    pt.BeginFrame(); pt.Compute()                                                # pins state C: the skin must write elsewhere
    want = R.skin(case["un"], case["joints"], pos, c, *case["args"])
    pt.Skin(*case["args"]); pt.synchronize()
    _assert_state(_download(pt, nv), want, "whole table")
    pt.Dispose()


@pytest.mark.parametrize("name", ["j_mirror", "w_subnormal", "r_ends_at_both_tables"])
def test_both_members_of_a_two_member_context_hold_the_restatement(name, native_builder):
    case = A.BY_NAME[name]
    sc = A.scene(case, native_builder); nv = len(sc.vertices)
    pt, pos, verts = _context(case, sc, devices=[0, 0])
    want = R.skin(case["un"], case["joints"], pos, verts, *case["args"])
    pt.Skin(*case["args"]); pt.synchronize()
    for member in (0, 1):
        pt.set_option("download_member", member)
        _assert_state(_download(pt, nv), want, (name, member))
    with pytest.raises(IdkPtError):
        pt.set_option("download_member", 2)
    pt.Dispose()


@pytest.mark.parametrize("use_tlas", [0, 1])
@pytest.mark.parametrize("name", A.FRAME_CASES)
def test_frames_after_a_skin_equal_the_oracle_on_a_host_scene_of_the_restatement(name, use_tlas, oracle_mod, native_builder, oracle_builder):
    """96 x 64, RayDepth 3, one sample.  The oracle's scene is built from the restatement and oracle_builder alone: positions, vertices, nodes and TLAS; nothing is downloaded into it."""
    case = A.BY_NAME[name]
    sc = A.scene(case, native_builder); nv = len(sc.vertices)
    w, h = 96, 64; cam = S.Camera(w, h, position=(0.0, 0.25, 7.0), fovy_deg=55.0)
    pt, pos, verts = _context(case, sc, poison=False, size=(w, h))
    pt.SetCamera(cam); pt.UseTlas = use_tlas; pt.RayDepth = 3
    pt.Skin(*case["args"]); pt.RefitBlas(1)
    if use_tlas:
        pt.BuildTlasOnDevice()
    pt.ResetAccumulation(); pt.Compute()
    want = R.skin(case["un"], case["joints"], pos, verts, *case["args"])
    assert np.isfinite(want[0]).all()
    host = copy.copy(sc)
    host.vertex_positions = np.ascontiguousarray(want[0], np.float32); host.vertices = want[2]; host.blas_nodes = _refit_want(sc, want[0], oracle_builder)
    host.mesh_transforms = sc.mesh_transforms.copy()
    S.rebuild_tlas(host, oracle_builder)
    o = oracle_render(oracle_mod, host, cam, w, h, RayDepth=3, UseTlas=use_tlas)
    image = o.image(0); o.close()
    assert (bits(pt.Result) == bits(image)).all(), (name, use_tlas)
    _assert_state(_download(pt, nv), want, name)                                 # (afterwards, and only compared: the frame above never saw these downloads)
    assert pt.DownloadBuffer(T.IDKPT_BUF_BLAS_NODES, T.GpuBlasNode, len(sc.blas_nodes)).tobytes() == host.blas_nodes.tobytes()
    if use_tlas:
        assert pt.DownloadBuffer(T.IDKPT_BUF_TLAS_NODES, T.GpuTlasNode, len(host.tlas_nodes)).tobytes() == host.tlas_nodes.tobytes()
    assert (image[..., :3] != np.float32([0.7, 0.8, 1.0])).any(-1).mean() > 0.05, "the frame shows the mesh, not only sky"
    pt.Dispose()
