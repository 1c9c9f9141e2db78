"""What temporal reprojection costs and gives on the device (profiles/reproject.md).
  * Time: idkptCaptureGeometry and idkptReproject at 1920 x 1080 and 3840 x 2160 on the soup headline view (bench.py's scene and camera), by HIP events on the context's
    stream, beside ONE tiled idkptDenoise iteration and a 16 B per pixel copy from the same run.  Warmed up, median / min / max of --reps calls.
  * Quality: the 64 x 64 Cornell box against a 4096-sample render of the moved camera: RMSE of a 1-sample frame after a small camera move, without history and with
    eight frames of history (eight 1-sample frames along the move, each reprojected onto the one before), for a few PositionTolerance / MaxHistory pairs.

    python tools/reproject_timing.py [--tris 1000000 --reps 20 --reference-samples 4096]"""
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
    ap.add_argument("--tris", type=int, default=1000000); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--reference-samples", type=int, default=4096)
    a = ap.parse_args()
    res = {"tris": a.tris, "reps": a.reps, "time": [], "quality": []}

    def timed(stream, fn, reps):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return [round(float(np.median(out)), 4), round(float(np.min(out)), 4), round(float(np.max(out)), 4)]

    sc = S.soup_scene(a.tris, NativeBuilder(), seed=1)
    for w, h in ((1920, 1080), (3840, 2160)):
        pt = PathTracer(w, h)
        pt.OutputAOVs = 1; pt.RayDepth = 2
        pt.UploadScene(sc); pt.SetFrameRing(2)
        st = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(st)))
        stream = torch.cuda.ExternalStream(st.value)
        cam_a = S.Camera(w, h); cam_b = S.Camera(w, h, position=(0.3, 0.1, 25.0), view_dir=(0.02, 0.0, -1.0))
        pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute(); pt.CaptureGeometry(); pt.Reproject(0, T.IDKPT_NO_HISTORY)
        pt.BeginFrame(); pt.SetCamera(cam_b); pt.Compute(); pt.synchronize()
        s = T.Reproject.from_camera(cam_a)
        d1 = T.Denoise(Iterations=1)
        capture = lambda: pt.CaptureGeometry()                                                   # noqa: E731
        reproject = lambda: pt._check(pt._L.idkptReproject(pt._ctx, 1, 0, C.addressof(s)))       # noqa: E731
        denoise1 = lambda: pt._check(pt._L.idkptDenoise(pt._ctx, 1, C.addressof(d1)))            # noqa: E731
        for fn in (capture, reproject, denoise1):
            for _ in range(3):
                fn()
        row = {"width": w, "height": h}
        for rnd in range(2):                                                                     # alternating, twice: the second round shows the run-to-run spread
            for name, fn in (("capture_ms", capture), ("reproject_ms", reproject), ("denoise_1_tiled_iteration_ms", denoise1)):
                row.setdefault(name, []).append(timed(stream, fn, a.reps))
        src = torch.empty(w * h * 4, dtype=torch.float32, device="cuda"); dst = torch.empty_like(src)
        with torch.cuda.stream(stream):
            for _ in range(3):
                dst.copy_(src)
            row["copy_16B_per_pixel_ms"] = timed(stream, lambda: dst.copy_(src), a.reps)
        row["history_fraction"] = round(float((pt.DownloadTemporal(1)[..., 3] > 1.0).mean()), 4)
        row["miss_fraction"] = round(float((pt.DownloadGeometry(1)[..., 3].view(np.uint32) == 0xFFFFFFFF).mean()), 4)
        res["time"].append(row)
        pt.Dispose()
        del src, dst

    # ---- quality on the small Cornell box
    w = h = 64
    box = S.cornell_scene(NativeBuilder(), variant="mixed")

    def cam(t):                                                                                  # the move: 0.02 along x and 0.4 degrees of yaw per frame
        return S.Camera(w, h, position=(0.02 * t, 0.0, 3.4), view_dir=(np.sin(np.radians(0.4 * t)), 0.0, -np.cos(np.radians(0.4 * t))), fovy_deg=40.0)

    ref = PathTracer(w, h); ref.RayDepth = 4; ref.UploadScene(box); ref.SetCamera(cam(8)); ref.set_max_batch(32)
    for _ in range(a.reference_samples):
        ref.Compute()
    truth = ref.Result[..., :3].astype(np.float64); ref.Dispose()
    rmse = lambda img: float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - truth) ** 2)))  # noqa: E731
    for tol, cap in ((0.02, 32.0), (0.005, 32.0), (0.1, 32.0), (0.02, 8.0), (0.02, 128.0)):
        pt = PathTracer(w, h); pt.RayDepth = 4; pt.UploadScene(box); pt.SetFrameRing(2)
        prev_cam, prev_slot = None, T.IDKPT_NO_HISTORY
        for t in range(9):                                                                       # frames 0..7 are the history, frame 8 is the one that is judged
            slot = pt.BeginFrame(); pt.SetCamera(cam(t)); pt.Compute(); pt.CaptureGeometry()
            pt.Reproject(slot, prev_slot, T.Reproject.from_camera(prev_cam, PositionTolerance=tol, MaxHistory=cap) if prev_cam is not None else None)
            prev_cam, prev_slot = cam(t), slot
        temporal = pt.DownloadTemporal(prev_slot)
        res["quality"].append({"PositionTolerance": tol, "MaxHistory": cap, "rmse_1_sample": round(rmse(pt.FrameResult(prev_slot)), 5), "rmse_with_8_frames_of_history": round(rmse(temporal), 5),
                               "mean_effective_samples": round(float(temporal[..., 3].mean()), 3), "pixels_with_history": round(float((temporal[..., 3] > 1.0).mean()), 4)})
        pt.Dispose()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
