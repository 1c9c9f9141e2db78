"""Motion-aware capture on the device: idkptCaptureMotion, its previous vertex positions (IDKPT_BUF_MOTION_PREV_POSITIONS) and idkptReproject / idkptReprojectMoments
through the motion image (csrc/kernels_reproject.hpp, csrc/host_reproject.hpp, csrc/host_scene.hpp; the contract: include/idkpt.h, "motion-aware capture").  Everything is
bit for bit: the motion image against the restated record (tests/motion_ref.py) of idkptTraceRays hits for centre rays made with the oracle's GetWorldSpaceDirection and of
the triangles uploaded, the downloaded previous positions and the downloaded transforms; the temporal images against the restated reprojection fed the downloaded images.

The scene is the Cornell box as three refittable BLASes (walls, short box, tall box) under a sky, seen from outside its open side.  The camera, the short box's move and the
tall box's skinning offset were chosen on the CPU from oracle hits so that the restatement alone shows what each case must show (the conditions asserted below on
restated data before anything is compared): every class of pixel at least 2 % of the frame; no history on the moved box without the motion image — the move has a
component across every face that exceeds the position tolerance — and history on at least half of it with."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import reproject_ref as R  # noqa: E402
import motion_ref as MR  # noqa: E402
from test_gpu_present import read_device  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from idkengine_amd._lib import IdkPtError  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
GUARD = 64
SIZES = [(64, 64), (70, 37)]                       # whole 16 x 16 tiles; no multiple of 16 or of 8 in either axis
SKY = (0.4, 0.6, 0.9)
CAM = dict(position=(0.0, 0.0, 3.4), view_dir=(0.0, 0.0, -1.0), fovy_deg=50.0)
SHORT, TALL = 1, 2                                 # BLAS, instance and GpuMeshTransform index of the two boxes (0: the walls)
MOVE = (0.07, 0.09, 0.08)                          # world translation of the short box between two frames: about two pixels, and across every one of its faces
SKIN_SHIFT = (0.05, 0.1, -0.04)                    # the joint's translation, in the tall box's local space
XFORM_BYTES = T.GpuMeshTransform.itemsize


@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, instanced=True, sky_color=SKY, refittable=True)


@pytest.fixture(scope="module")
def ray_program(tmp_path_factory):
    """the oracle's GetWorldSpaceDirection as a program (tests/c_driver/reproject_host.cpp; no sanitizer here: tests/test_reproject_ref.py runs it under ASan/UBSan)"""
    return R.build_host_program(str(tmp_path_factory.mktemp("motion_rays") / "reproject_host"), sanitize=False)


def new_pt(sc, w, h, ring=2, noise=False, **kw):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(w, h, **kw)
    pt.OutputAOVs = 1; pt.RayDepth = 3; pt.UseTlas = True
    pt.UploadScene(sc)
    if ring > 1:
        pt.SetFrameRing(ring)
    if noise:
        pt.SetNoiseEstimate(True)
    return pt


def vertex_range(sc, blas):
    """[first, end) of the vertices the triangles of BLAS `blas` use (assemble lays the meshes out BLAS by BLAS)"""
    d = sc.blas_descs[blas]
    t = sc.blas_triangles[d["TriangleOffset"]: d["TriangleOffset"] + d["TriangleCount"]]
    ids = np.concatenate([t["X"], t["Y"], t["Z"]])
    return int(ids.min()), int(ids.max()) + 1


def moved_transform(sc, index, world_shift):
    """GpuMeshTransform `index` translated by world_shift, its PrevModel the Model it had"""
    old = sc.mesh_transforms[index: index + 1]
    m = np.eye(4); m[:3, :3] = old["Model"][0][:, :3].T.astype(np.float64); m[3, :3] = old["Model"][0][:, 3]
    new = S.transform_from_matrix(m @ S.translation(world_shift))
    new["PrevModel"] = old["Model"]
    return new


def move_short_box(pt, sc):
    pt.UpdateBuffer(T.IDKPT_BUF_MESH_TRANSFORMS, moved_transform(sc, SHORT, MOVE), offset_bytes=SHORT * XFORM_BYTES)
    pt.BuildTlasOnDevice()


def skin_tall_box(pt, sc, shift):
    """the tall box's vertices bound to one joint that translates them by `shift`; returns their range"""
    first, end = vertex_range(sc, TALL)
    un = np.zeros(end - first, T.GpuUnskinnedVertex)
    un["JointWeights"][:, 0] = 1.0; un["Position"] = sc.vertex_positions.reshape(-1, 3)[first:end]
    un["Tangent"] = sc.vertices["Tangent"][first:end]; un["Normal"] = sc.vertices["Normal"][first:end]
    joint = np.zeros((1, 3, 4), np.float32); joint[0, :, :3] = np.eye(3); joint[0, :, 3] = shift
    pt.UploadUnskinnedVertices(un); pt.UpdateBuffer(T.IDKPT_BUF_JOINT_MATRICES, joint)
    pt.Skin(0, first, 0, end - first); pt.RefitBlas(TALL)
    return first, end


def triangles(sc):
    return np.stack([sc.blas_triangles[k] for k in ("X", "Y", "Z", "MeshId")], -1).astype(np.uint32)


def positions(pt, sc):
    return pt.DownloadBuffer(T.IDKPT_BUF_VERTEX_POSITIONS, np.float32, len(sc.vertices) * 3).reshape(-1, 3)


def image_and_guard(pt, ptr_fn, download, slot):
    p, n = ptr_fn(slot)
    assert n == pt.height * pt.width * 16
    raw = read_device(pt, p, n + GUARD)
    body = raw[:n].view(np.float32).reshape(pt.height, pt.width, 4)
    assert R.same(body, download(slot))                   # the device pointer equals the download
    return body, raw[n:]


def guards_intact(pt, slots, motion=True, temporal=True, moments=False):
    for q in slots:
        pairs = [(pt.geometry_device_ptr, pt.DownloadGeometry)]
        pairs += [(pt.motion_device_ptr, pt.DownloadMotion)] if motion else []
        pairs += [(pt.temporal_device_ptr, pt.DownloadTemporal)] if temporal else []
        pairs += [(pt.temporal_moments_device_ptr, pt.DownloadTemporalMoments)] if moments else []
        for ptr_fn, download in pairs:
            assert (image_and_guard(pt, ptr_fn, download, q)[1] == 0xA5).all()
    return True


def traced_centre_hits(pt, ray_program, tmp, cam, W, H):
    o, d = R.oracle_centre_rays(ray_program, str(tmp), cam.inv_projection, cam.inv_view, W, H)
    rays = np.zeros(W * H, T.RayQuery); rays["Origin"] = o; rays["Direction"] = d.reshape(-1, 3); rays["MaxDist"] = R.FLT_MAX
    return o, d, pt.TraceRays(rays)


def restated_images(pt, sc, o, d, hits, W, H):
    """(geometry, motion) restated from traced hits, the uploaded triangles and what the context holds of previous positions and transforms"""
    g = R.pack(o, d, hits["T"].reshape(H, W), hits["MeshTransformId"].reshape(H, W), hits["Hit"].reshape(H, W))
    xf = pt.DownloadBuffer(T.IDKPT_BUF_MESH_TRANSFORMS, T.GpuMeshTransform, len(sc.mesh_transforms))
    return g, MR.motion_image(g, hits, triangles(sc), pt.DownloadMotionPrevPositions(len(sc.vertices)), xf["PrevModel"])


# ---- 1. the record
@pytest.mark.parametrize("size", SIZES, ids=["64x64", "70x37"])
def test_motion_image_equals_the_restated_record(scene, ray_program, tmp_path, size):
    W, H = size
    pt = new_pt(scene, W, H)
    cam = S.Camera(W, H, **CAM)
    pt.BeginFrame(); pt.SetCamera(cam); pt.Compute()
    pt.CaptureMotion()                                    # the first capture: the previous positions become the positions
    move_short_box(pt, scene)
    first, end = skin_tall_box(pt, scene, SKIN_SHIFT)
    pt.BuildTlasOnDevice()
    slot = pt.BeginFrame(); pt.Compute(); pt.CaptureMotion()
    o, d, hits = traced_centre_hits(pt, ray_program, tmp_path, cam, W, H)
    want_g, want_m = restated_images(pt, scene, o, d, hits, W, H)
    # conditions, on the restatement alone: moved-instance, skinned, static and miss pixels are each at least 2 % of the frame, and the two kinds of motion show
    hit = hits["Hit"].reshape(H, W) != 0; ids = hits["MeshTransformId"].reshape(H, W)
    share = {"moved": (hit & (ids == SHORT)).mean(), "skinned": (hit & (ids == TALL)).mean(), "static": (hit & (ids == 0)).mean(), "miss": (~hit).mean()}
    assert all(v >= 0.02 for v in share.values()), share
    apart = np.sqrt(((want_m[..., :3] - want_g[..., :3]).astype(np.float64) ** 2).sum(-1))
    for k, shift in ((SHORT, MOVE), (TALL, SKIN_SHIFT)):
        sel = hit & (ids == k)
        assert np.allclose(apart[sel], np.linalg.norm(shift), rtol=1e-3), k          # every pixel of a mover stood its move away
    assert (apart[hit & (ids == 0)] < 1e-5).all() and R.same(want_m[~hit], want_g[~hit])
    prev = pt.DownloadMotionPrevPositions(len(scene.vertices)); now = positions(pt, scene)
    assert not R.same(prev[first:end], now[first:end]) and R.same(prev[:first], now[:first])
    # the device
    got_g, guard_g = image_and_guard(pt, pt.geometry_device_ptr, pt.DownloadGeometry, slot)
    got_m, guard_m = image_and_guard(pt, pt.motion_device_ptr, pt.DownloadMotion, slot)
    assert R.same(got_m, want_m), int((R.bits(got_m) != R.bits(want_m)).any(axis=2).sum())
    assert R.same(got_g, want_g)
    assert (guard_g == 0xA5).all() and (guard_m == 0xA5).all()
    pt.CaptureGeometry()                                  # the same state through idkptCaptureGeometry: the same geometry image, and the motion image is dropped
    assert R.same(pt.DownloadGeometry(slot), got_g)
    buf = np.zeros((H, W, 4), np.float32); p = C.c_void_p(); n = C.c_size_t()
    assert pt._L.idkptDownloadMotion(pt._ctx, slot, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION and pt._L.idkptGetMotionDevicePtr(pt._ctx, slot, C.byref(p), C.byref(n)) == INVALID_OPERATION
    assert R.same(pt.DownloadMotion(1 - slot)[..., 3], pt.DownloadGeometry(1 - slot)[..., 3])          # (the other slot keeps its own)
    pt.Dispose()


# ---- 2. the previous positions
def test_previous_positions_follow_the_skin(scene):
    W, H = 64, 64
    pt = new_pt(scene, W, H)
    nv = len(scene.vertices)
    pt.SetCamera(S.Camera(W, H, **CAM))
    with pytest.raises(IdkPtError):
        pt.DownloadMotionPrevPositions(nv)                # before the first capture
    out = np.zeros(nv * 3, np.float32)
    assert pt._L.idkptDownloadBuffer(pt._ctx, T.IDKPT_BUF_MOTION_PREV_POSITIONS, 0, out.nbytes, out.ctypes.data) == INVALID_OPERATION
    original = positions(pt, scene)
    assert R.same(original, scene.vertex_positions.reshape(-1, 3))
    pt.CaptureMotion()
    assert R.same(pt.DownloadMotionPrevPositions(nv), original)                               # the first capture: a copy of the positions
    assert pt._L.idkptDownloadBuffer(pt._ctx, T.IDKPT_BUF_MOTION_PREV_POSITIONS, 12, out.nbytes, out.ctypes.data) == INVALID_ARGUMENT   # a range past the end
    first, end = skin_tall_box(pt, scene, SKIN_SHIFT)
    skinned1 = positions(pt, scene)
    assert not R.same(skinned1[first:end], original[first:end]) and R.same(skinned1[:first], original[:first]) and R.same(skinned1[end:], original[end:])
    assert R.same(pt.DownloadMotionPrevPositions(nv), original)                               # inside the range: the replaced positions; outside: untouched
    old_prev = pt.DownloadBuffer(T.IDKPT_BUF_PREV_VERTEX_POSITIONS, np.float32, nv * 3).reshape(-1, 3)
    assert R.same(old_prev[first:end], original[first:end]) and (old_prev[:first] == 0).all() and (old_prev[end:] == 0).all()   # idkptSkin's own record is as it was
    half = first + (end - first) // 2                                                          # a second skin of the first half of the range, another joint
    joint = np.zeros((1, 3, 4), np.float32); joint[0, :, :3] = np.eye(3); joint[0, :, 3] = (-0.02, 0.0, 0.03)
    pt.UpdateBuffer(T.IDKPT_BUF_JOINT_MATRICES, joint); pt.Skin(0, first, 0, half - first)
    prev2 = pt.DownloadMotionPrevPositions(nv)
    assert R.same(prev2[first:half], skinned1[first:half]) and R.same(prev2[half:], original[half:]) and R.same(prev2[:first], original[:first])   # the first skin's output
    assert not R.same(positions(pt, scene)[first:half], skinned1[first:half])
    # idkptUpdateBuffer of positions does not write them; idkptUploadScene re-creates them from the new positions
    before = pt.DownloadMotionPrevPositions(nv)
    pt.UpdateBuffer(T.IDKPT_BUF_VERTEX_POSITIONS, original + np.float32(0.25))
    assert R.same(pt.DownloadMotionPrevPositions(nv), before)
    pt.UploadScene(scene)
    assert R.same(pt.DownloadMotionPrevPositions(nv), original)
    pt.Dispose()


# ---- 3. history follows the mover
def mover_sequence(pt, sc, cam, motion, n0=4, n1=1, one_more=False):
    """frame 0, the short box moves, frame 1 reprojected onto frame 0 (colour and moments); returns what the restatement needs and what the device made.
    one_more: a further sample of frame 0 behind its reprojection — under set_max_batch it is still queued, reading the transforms, when the move rewrites them"""
    capture = pt.CaptureMotion if motion else pt.CaptureGeometry
    sa = T.Reproject.from_camera(cam)
    assert pt.BeginFrame() == 0
    pt.SetCamera(cam)
    for _ in range(n0):
        pt.Compute()
    capture(); pt.Reproject(0, T.IDKPT_NO_HISTORY); pt.ReprojectMoments(0, T.IDKPT_NO_HISTORY)
    if one_more:
        pt.Compute()
    move_short_box(pt, sc)
    assert pt.BeginFrame() == 1
    for _ in range(n1):
        pt.Compute()
    capture(); pt.Reproject(1, 0, sa); pt.ReprojectMoments(1, 0, sa)
    out = dict(result=pt.FrameResult(1), mom=pt.DownloadMoments(1), g=pt.DownloadGeometry(1), hg=pt.DownloadGeometry(0), hc=pt.DownloadTemporal(0), hm=pt.DownloadTemporalMoments(0),
               temporal=pt.DownloadTemporal(1), tmoments=pt.DownloadTemporalMoments(1), accumulated=[pt.FrameResult(q, i) for q in (0, 1) for i in range(3)])
    out["l"] = pt.DownloadMotion(1) if motion else out["g"]
    return out


@pytest.mark.parametrize("size", SIZES, ids=["64x64", "70x37"])
def test_history_follows_a_moving_box(scene, size):
    W, H = size
    cam = S.Camera(W, H, **CAM)
    M = (cam.view @ cam.proj).astype(np.float32)
    n1 = 1
    for motion in (False, True):
        pt = new_pt(scene, W, H, noise=True)
        s = mover_sequence(pt, scene, cam, motion, n1=n1)
        box = R.bits(s["g"][..., 3]) == SHORT
        assert box.mean() >= 0.02
        st = {}
        want = MR.reproject(s["result"], n1, s["g"], s["l"], s["hg"], s["hc"], M, cam.position, stats=st, **R.DEFAULTS)
        want_m = MR.reproject_moments(s["mom"], n1, s["g"], s["l"], s["hg"], s["hm"], M, cam.position, **R.DEFAULTS)
        if not motion:
            assert R.same(want, R.reproject(s["result"], n1, s["g"], s["hg"], s["hc"], M, cam.position, **R.DEFAULTS))   # the restatement of the parent's contract
            assert (want[..., 3][box] == np.float32(n1)).all() and not st["history"][box].any()    # the parent's behaviour: the moved box starts over, every pixel of it
        else:
            assert st["history"][box].mean() >= 0.5, st["history"][box].mean()                     # the condition, on the restatement alone
            assert (want[..., 3][box & st["history"]] > np.float32(n1)).all()
        assert st["history"][~box].mean() >= 0.5
        assert R.same(s["temporal"], want), int((R.bits(s["temporal"]) != R.bits(want)).any(axis=2).sum())
        assert R.same(s["tmoments"], want_m), int((R.bits(s["tmoments"]) != R.bits(want_m)).any(axis=2).sum())
        assert R.same(s["tmoments"][..., 3], s["temporal"][..., 3])                                # the moments' count is the temporal alpha
        assert R.same(pt.DownloadTemporal(0), s["hc"]) and R.same(pt.DownloadGeometry(0), s["hg"])   # the history is read, not written
        assert guards_intact(pt, (0, 1), motion=motion, moments=True)
        pt.Dispose()


# ---- 4. a static scene
@pytest.mark.parametrize("size", SIZES, ids=["64x64", "70x37"])
def test_static_records_lie_within_the_tolerance_and_capture_geometry_restores_the_old_path(scene, size):
    W, H = size
    cam_a = S.Camera(W, H, **CAM); cam_b = S.Camera(W, H, position=(0.15, 0.05, 3.3), view_dir=(-0.04, 0.0, -1.0), fovy_deg=50.0)
    a, b = new_pt(scene, W, H), new_pt(scene, W, H)
    for pt, motion in ((a, True), (b, False)):
        pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute(); pt.Compute()
        (pt.CaptureMotion if motion else pt.CaptureGeometry)(); pt.Reproject(0, T.IDKPT_NO_HISTORY)
        pt.BeginFrame(); pt.SetCamera(cam_b); pt.Compute()
        (pt.CaptureMotion if motion else pt.CaptureGeometry)()
    g, m = a.DownloadGeometry(1), a.DownloadMotion(1)
    hit = R.bits(g[..., 3]) != 0xFFFFFFFF
    assert hit.mean() > 0.3 and (~hit).any() and R.same(m[~hit], g[~hit]) and R.same(m[..., 3], g[..., 3])
    with np.errstate(all="ignore"):                       # each hit pixel's motion record lies within its own limit of its geometry record
        tol2 = np.float32(np.float32(0.02) * np.float32(0.02))
        limit = tol2 * MR._d2(m[..., 0], m[..., 1], m[..., 2], *np.float32(cam_a.position))
        assert (MR._d2(m[..., 0], m[..., 1], m[..., 2], g[..., 0], g[..., 1], g[..., 2])[hit] <= limit[hit]).all()
    sa = T.Reproject.from_camera(cam_a)
    a.Reproject(1, 0, sa); b.Reproject(1, 0, sa)
    through_motion, plain = a.DownloadTemporal(1), b.DownloadTemporal(1)
    assert (plain[..., 3] > 1.0).mean() >= 0.5 and (through_motion[..., 3] > 1.0).mean() >= 0.5   # (both find history; they may differ by a rounding of the position)
    a.CaptureGeometry()                                  # drops the motion image: idkptReproject runs what it ran before, bit for bit
    a.Reproject(1, 0, sa)
    assert R.same(a.DownloadTemporal(1), plain) and R.same(a.DownloadGeometry(1), b.DownloadGeometry(1))
    assert guards_intact(a, (0, 1), motion=False) and guards_intact(b, (0, 1), motion=False)
    a.Dispose(); b.Dispose()


# ---- 5. additive: the accumulated images and the count never notice
def test_the_accumulation_is_bit_identical_with_and_without_the_new_calls(scene):
    W, H = 70, 37
    cam = S.Camera(W, H, **CAM)
    with_calls, without = new_pt(scene, W, H), new_pt(scene, W, H)
    for pt, calls in ((with_calls, True), (without, False)):
        pt.set_max_batch(2)                               # (samples stay queued between calls: the new calls launch them first)
        pt.BeginFrame(); pt.SetCamera(cam)
        pt.Compute(); pt.Compute(); pt.Compute()
        if calls:
            pt.CaptureMotion(); pt.Reproject(0, T.IDKPT_NO_HISTORY)
        pt.Compute()
        move_short_box(pt, scene); skin_tall_box(pt, scene, SKIN_SHIFT); pt.BuildTlasOnDevice()
        pt.BeginFrame()
        pt.Compute()
        if calls:
            pt.CaptureMotion(); pt.Reproject(1, 0, T.Reproject.from_camera(cam)); pt.DownloadMotion(1)
        pt.Compute(); pt.Compute()
        if calls:
            pt.CaptureMotion(); pt.Reproject(1, 0, T.Reproject.from_camera(cam))
    for slot in (0, 1):
        for image in range(3):
            assert R.same(with_calls.FrameResult(slot, image), without.FrameResult(slot, image)), (slot, image)
    assert with_calls.AccumulatedSamples == without.AccumulatedSamples == 3
    assert np.abs(with_calls.FrameResult(1, 1)[..., :3]).max() > 0
    nv = len(scene.vertices)
    assert R.same(positions(with_calls, scene), positions(without, scene))
    assert R.same(with_calls.DownloadBuffer(T.IDKPT_BUF_PREV_VERTEX_POSITIONS, np.float32, nv * 3), without.DownloadBuffer(T.IDKPT_BUF_PREV_VERTEX_POSITIONS, np.float32, nv * 3))
    assert guards_intact(with_calls, (0, 1))
    for pt in (with_calls, without):
        pt.Dispose()


# ---- 6. scene versions
def test_scene_versions_do_not_change_a_bit(scene):
    W, H = 70, 37
    cam = S.Camera(W, H, **CAM)
    for one_more in (False, True):                        # the sequence of the case above, and the same with a sample of frame 0 still queued when the transform is rewritten
        runs = []
        for versions in (1, 2):
            pt = new_pt(scene, W, H, noise=True)
            pt.SetSceneVersions(versions); pt.set_max_batch(2)
            runs.append(mover_sequence(pt, scene, cam, True, n0=3, n1=2, one_more=one_more))
            assert guards_intact(pt, (0, 1), moments=True)
            pt.Dispose()
        one, two = runs
        for k in ("g", "l", "hg", "hc", "hm", "temporal", "tmoments", "result", "mom"):
            assert R.same(one[k], two[k]), (k, one_more)
        for x, y in zip(one["accumulated"], two["accumulated"]):
            assert R.same(x, y)
        box = R.bits(one["g"][..., 3]) == SHORT
        assert (one["temporal"][..., 3][box] > 2.0).mean() >= 0.5        # (and the sequence still follows the box)


# ---- 7. refusals, before anything is launched
def test_refusals(scene):
    from idkengine_amd import _lib
    from idkengine_amd.pathtracer import PathTracer
    W, H = 64, 64
    cam = S.Camera(W, H, **CAM)
    buf = np.zeros((H, W, 4), np.float32); p = C.c_void_p(); n = C.c_size_t()
    L = _lib.load()
    raw = C.c_void_p()
    assert L.idkptCreate(1, (C.c_int32 * 1)(0), C.byref(raw)) == 0                                   # no size set
    assert L.idkptCaptureMotion(raw, -1) == INVALID_OPERATION and L.idkptDownloadMotion(raw, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
    assert L.idkptDestroy(raw) == 0
    bare = PathTracer(W, H)
    assert bare._L.idkptCaptureMotion(bare._ctx, -1) == INVALID_OPERATION                          # no scene uploaded
    out = np.zeros(3, np.float32)
    assert bare._L.idkptDownloadBuffer(bare._ctx, T.IDKPT_BUF_MOTION_PREV_POSITIONS, 0, 12, out.ctypes.data) == INVALID_OPERATION
    bare.Dispose()
    pt = new_pt(scene, W, H)
    pt.SetCamera(cam); pt.Compute()
    ctx = pt._ctx
    for q in (-2, 2, 7):                                                                            # a slot outside the ring
        assert L.idkptCaptureMotion(ctx, q) == INVALID_ARGUMENT and L.idkptDownloadMotion(ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_ARGUMENT
        assert L.idkptGetMotionDevicePtr(ctx, q, C.byref(p), C.byref(n)) == INVALID_ARGUMENT
    for q in (-1, 0, 1):                                                                            # a motion download before any capture, and after a geometry capture
        assert L.idkptDownloadMotion(ctx, q, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION and L.idkptGetMotionDevicePtr(ctx, q, C.byref(p), C.byref(n)) == INVALID_OPERATION
    pt.CaptureGeometry()
    assert L.idkptDownloadMotion(ctx, 0, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
    with pytest.raises(IdkPtError):
        pt.DownloadMotionPrevPositions(len(scene.vertices))                                         # (idkptCaptureGeometry allocates no previous positions)
    pt.CaptureMotion()
    kept = pt.DownloadMotion(0)
    for nbytes in (buf.nbytes - 16, buf.nbytes + 16, 0):
        assert L.idkptDownloadMotion(ctx, 0, buf.ctypes.data, nbytes) == INVALID_ARGUMENT
    assert L.idkptDownloadMotion(ctx, 0, None, buf.nbytes) == INVALID_ARGUMENT and L.idkptGetMotionDevicePtr(ctx, 0, None, None) == INVALID_ARGUMENT
    assert L.idkptCaptureMotion(ctx, 2) == INVALID_ARGUMENT and R.same(pt.DownloadMotion(0), kept) and guards_intact(pt, (0,), temporal=False)
    pt.Dispose()
    for kw in (dict(devices=[0, 0]), dict(row_modulo=2, row_remainder=1, row_band=8)):               # a member context, a row shard
        pt = PathTracer(W, H, **kw)
        pt.UploadScene(scene); pt.SetCamera(cam); pt.Compute()
        assert pt._L.idkptCaptureMotion(pt._ctx, -1) == INVALID_OPERATION and pt._L.idkptDownloadMotion(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION
        assert pt._L.idkptGetMotionDevicePtr(pt._ctx, -1, C.byref(p), C.byref(n)) == INVALID_OPERATION
        assert pt._L.idkptDownloadBuffer(pt._ctx, T.IDKPT_BUF_MOTION_PREV_POSITIONS, 0, 12, out.ctypes.data) == INVALID_OPERATION
        pt.Dispose()


# ---- lifetime: the motion image goes and stays with the slot's other images
def test_the_motion_image_survives_the_reset_and_goes_with_the_size(scene):
    W, H = 64, 64
    cam = S.Camera(W, H, **CAM)
    pt = new_pt(scene, W, H)
    pt.BeginFrame(); pt.SetCamera(cam); pt.Compute(); pt.CaptureMotion()
    kept = pt.DownloadMotion(0)
    pt.ResetAccumulation(); pt.set_max_batch(4); pt.SetPresentationSize(32, 32)
    assert R.same(pt.DownloadMotion(0), kept)
    buf = np.zeros((H, W, 4), np.float32)

    def gone():
        assert pt._L.idkptDownloadMotion(pt._ctx, 0, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION

    def again():
        pt.SetCamera(cam); pt.Compute(); pt.CaptureMotion(0)
        assert R.same(pt.DownloadMotion(0), kept) and guards_intact(pt, (0,), temporal=False)

    pt.SetSize(W, H); gone(); again()
    pt.SetFrameRing(3); gone(); again()
    for call in (lambda: pt._L.idkptSetRowSharding(pt._ctx, 1, 0), lambda: pt._L.idkptSetRowBands(pt._ctx, 8, 1, 0), lambda: pt._L.idkptSetRowRange(pt._ctx, 0, H)):
        assert call() == 0
        gone(); again()
    pt.Dispose()
