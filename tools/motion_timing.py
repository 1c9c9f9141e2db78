"""What motion-aware capture costs and gives on the device (profiles/motion.md).
  * Time, by HIP events on the context's stream, warmed up, median / min / max of --reps calls, two alternating rounds (the second shows the run-to-run spread), at
    1920 x 1080: idkptCaptureMotion beside idkptCaptureGeometry, and idkptReproject of a slot with and without a motion image — on the soup headline view (bench.py's scene
    and camera) and on the procedural atrium as 87 BLASes.
  * Quality: the 64 x 64 Cornell box as three instances, its short box moving a little every frame; eight 1-sample frames of history, then the frame that is judged against a
    converged render of the final state.  RMSE on the box's pixels and on the pixels the box uncovered in the last step, with idkptCaptureGeometry and with idkptCaptureMotion.

    python tools/motion_timing.py [--tris 1000000 --atrium-tris 262000 --reps 20 --reference-samples 4096]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    import torch
    from idkengine_amd import scenes as S, gputypes as T
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1000000); ap.add_argument("--atrium-tris", type=int, default=262000)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--reference-samples", type=int, default=4096)
    a = ap.parse_args()
    res = {"reps": a.reps, "time": [], "quality": []}

    def timed(stream, fn, reps):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return [round(float(np.median(out)), 4), round(float(np.min(out)), 4), round(float(np.max(out)), 4)]

    w, h = 1920, 1080
    workloads = [("soup headline view", lambda: S.soup_scene(a.tris, NativeBuilder(), seed=1), lambda: S.Camera(w, h), lambda: S.Camera(w, h, position=(0.3, 0.1, 25.0), view_dir=(0.02, 0.0, -1.0))),
                 ("atrium, 87 BLASes", lambda: S.atrium_scene(a.atrium_tris, NativeBuilder(), per_mesh_blas=True), lambda: S.atrium_camera(w, h), lambda: S.atrium_camera(w, h))]
    for name, make, cam_a_of, cam_b_of in workloads:
        sc = make()
        pt = PathTracer(w, h)
        pt.OutputAOVs = 1; pt.RayDepth = 2
        pt.UploadScene(sc); pt.SetFrameRing(2)
        st = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(st)))
        stream = torch.cuda.ExternalStream(st.value)
        cam_a, cam_b = cam_a_of(), cam_b_of()
        pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute(); pt.CaptureGeometry(); pt.Reproject(0, T.IDKPT_NO_HISTORY)
        pt.BeginFrame(); pt.SetCamera(cam_b); pt.Compute(); pt.synchronize()
        s = T.Reproject.from_camera(cam_a)
        reproject = lambda: pt._check(pt._L.idkptReproject(pt._ctx, 1, 0, C.addressof(s)))       # noqa: E731
        row = {"workload": name, "width": w, "height": h, "instances": int(len(sc.blas_instances))}
        for _ in range(3):
            pt.CaptureGeometry(); reproject(); pt.CaptureMotion(); reproject()
        for rnd in range(2):
            row.setdefault("capture_geometry_ms", []).append(timed(stream, pt.CaptureGeometry, a.reps))
            row.setdefault("reproject_ms", []).append(timed(stream, reproject, a.reps))          # the slot holds no motion image here
            row.setdefault("capture_motion_ms", []).append(timed(stream, pt.CaptureMotion, a.reps))
            row.setdefault("reproject_through_motion_ms", []).append(timed(stream, reproject, a.reps))
        row["history_fraction"] = round(float((pt.DownloadTemporal(1)[..., 3] > 1.0).mean()), 4)
        row["miss_fraction"] = round(float((pt.DownloadGeometry(1)[..., 3].view(np.uint32) == 0xFFFFFFFF).mean()), 4)
        res["time"].append(row)
        pt.Dispose()

    # ---- quality on the small Cornell box with a moving box
    w = h = 64
    box = S.cornell_scene(NativeBuilder(), instanced=True, sky_color=(0.4, 0.6, 0.9))
    cam = S.Camera(w, h, position=(0.0, 0.0, 3.4), fovy_deg=50.0)
    step = np.array((0.035, 0.045, 0.04))                                                        # per frame: about a pixel, across every face of the box
    old = box.mesh_transforms[1:2]
    base = np.eye(4); base[:3, :3] = old["Model"][0][:, :3].T.astype(np.float64); base[3, :3] = old["Model"][0][:, 3]

    def transform(t):
        x = S.transform_from_matrix(base @ S.translation(step * t))
        x["PrevModel"] = S.transform_from_matrix(base @ S.translation(step * max(t - 1, 0)))["Model"]
        return x

    def new_pt(ring):
        pt = PathTracer(w, h); pt.RayDepth = 4; pt.UseTlas = True; pt.UploadScene(box)
        if ring > 1:
            pt.SetFrameRing(ring)
        pt.SetCamera(cam)
        return pt

    def place(pt, t):
        pt.UpdateBuffer(T.IDKPT_BUF_MESH_TRANSFORMS, transform(t), offset_bytes=T.GpuMeshTransform.itemsize); pt.BuildTlasOnDevice()

    ref = new_pt(1); place(ref, 8); ref.set_max_batch(32)
    for _ in range(a.reference_samples):
        ref.Compute()
    truth = ref.Result[..., :3].astype(np.float64)
    ref.CaptureGeometry(); on_box_now = ref.DownloadGeometry()[..., 3].view(np.uint32) == 1
    place(ref, 7); ref.CaptureGeometry(); on_box_before = ref.DownloadGeometry()[..., 3].view(np.uint32) == 1
    ref.Dispose()
    uncovered = on_box_before & ~on_box_now
    rmse = lambda img, m: float(np.sqrt(np.mean((img[..., :3].astype(np.float64)[m] - truth[m]) ** 2)))   # noqa: E731
    for motion in (False, True):
        pt = new_pt(2)
        prev_slot = T.IDKPT_NO_HISTORY
        for t in range(9):                                                                       # frames 0..7 are the history, frame 8 is the one that is judged
            place(pt, t)
            slot = pt.BeginFrame(); pt.Compute()
            (pt.CaptureMotion if motion else pt.CaptureGeometry)()
            pt.Reproject(slot, prev_slot, T.Reproject.from_camera(cam) if t else None)
            prev_slot = slot
        temporal, noisy = pt.DownloadTemporal(prev_slot), pt.FrameResult(prev_slot)
        everything = np.ones((h, w), bool)
        res["quality"].append({"capture": "motion" if motion else "geometry", "box_pixels": int(on_box_now.sum()), "uncovered_pixels": int(uncovered.sum()),
                               "rmse_1_sample": {"box": round(rmse(noisy, on_box_now), 5), "uncovered": round(rmse(noisy, uncovered), 5), "frame": round(rmse(noisy, everything), 5)},
                               "rmse_with_8_frames_of_history": {"box": round(rmse(temporal, on_box_now), 5), "uncovered": round(rmse(temporal, uncovered), 5), "frame": round(rmse(temporal, everything), 5)},
                               "mean_effective_samples_on_box": round(float(temporal[..., 3][on_box_now].mean()), 3),
                               "box_pixels_with_history": round(float((temporal[..., 3][on_box_now] > 1.0).mean()), 4)})
        pt.Dispose()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
