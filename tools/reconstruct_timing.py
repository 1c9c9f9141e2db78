"""What history reconstruction costs and gives (profiles/reconstruct.md).  Needs a GPU; prints one JSON object and writes it to --out.

Times, by HIP events around --reps calls after 3 warm-up calls, at 1920 x 1080 and 3840 x 2160 in one run, three rounds that alternate the calls: idkptReconstructHistory
(the starting values: Radius 2, Stride 3; one launch of k_reconstruct<2>) beside idkptReproject and idkptRectifyHistory (Radius 2; one launch of k_rectify<2>) over two
captures of the Cornell box, the protocol of tools/rectify_timing.py.  The reconstruction is timed under four loads of the same slot: the temporal counts planted to 8
(no pixel below FillBelow), the counts the camera move left (slot 0 holds six samples, slot 1 one sample reprojected onto it), the counts planted to 1 (every pixel below
FillBelow walks every tap and finds nobody who gives), and a checkerboard of 1 and 8 (half of the pixels walk, half of their taps give and fetch their guides).  The call
is in place and moves no count, so every repetition does the same work.

Quality: the 64 x 64 Cornell box and the camera move of profiles/reproject.md (0.02 along x and 0.4 degrees of yaw per frame), one sample per frame (frame k draws the
random numbers of sample k), two contexts that run the same frames, one with idkptReconstructHistory behind the three reprojections of every frame and one without.
Frame 8 is "the frame of the move" that is judged, then frames 9, 10 and 12, each against --reference-samples samples under its own camera: RMSE over rgb on the pixels
that were below FillBelow in frame 8 BEFORE the call (at the later frames: on the pixels below FillBelow in that frame) and on all pixels, of the temporal image and behind
idkptDenoiseTemporal.  One run; the five settings are the documented starting values: nothing is swept here."""
import argparse
import ctypes as C
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--reference-samples", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("reconstruct_timing needs a GPU")
    from idkengine_amd import _lib, gputypes as T, scenes as S
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    import reconstruct_ref as R
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    box = S.cornell_scene(NativeBuilder(), variant="mixed")
    res = {"reps": args.reps, "settings": R.DEFAULTS, "time": [], "quality": {}}
    fill = np.float32(R.DEFAULTS["FillBelow"])

    for W, H in ((1920, 1080), (3840, 2160)):
        pt = PathTracer(W, H)
        pt.RayDepth = 2; pt.OutputAOVs = 1
        pt.UploadScene(box); pt.SetFrameRing(2); pt.SetNoiseEstimate(True)
        st = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(st)))
        stream = torch.cuda.ExternalStream(st.value)
        cam_a = S.Camera(W, H, position=(0.0, 0.0, 3.4), view_dir=(0.0, 0.0, -1.0), fovy_deg=40.0)
        cam_b = S.Camera(W, H, position=(0.02, 0.0, 3.4), view_dir=(0.01, 0.0, -1.0), fovy_deg=40.0)
        pt.BeginFrame(); pt.SetCamera(cam_a)
        for _ in range(6):
            pt.Compute()
        pt.CaptureGeometry()
        pt.Reproject(0, T.IDKPT_NO_HISTORY); pt.ReprojectMoments(0, T.IDKPT_NO_HISTORY); pt.ReprojectFast(0, T.IDKPT_NO_HISTORY)
        pt.BeginFrame(); pt.SetCamera(cam_b); pt.Compute(); pt.CaptureGeometry(); pt.synchronize()
        s = T.Reproject.from_camera(cam_a); sf = T.Reproject.from_camera(cam_a, MaxHistory=4.0)
        pt.Reproject(1, 0, s); pt.ReprojectMoments(1, 0, s); pt.ReprojectFast(1, 0, sf)

        def timed(fn, reps=args.reps):
            with torch.cuda.stream(stream):
                for _ in range(3):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    fn()
                e1.record(stream)
            e1.synchronize()
            return round(e0.elapsed_time(e1) / reps, 4)

        def write_temporal(img):
            holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (H, W, 4), "typestr": "<f4", "data": (int(pt.temporal_device_ptr(1)[0]), False), "version": 2}})()
            with torch.cuda.stream(stream):
                torch.as_tensor(holder, device="cuda").copy_(torch.from_numpy(np.ascontiguousarray(img, np.float32)).to("cuda"))
            stream.synchronize()

        moved = pt.DownloadTemporal(1)
        hit = R.bits(pt.DownloadGeometry(1)[..., 3]) != R.MISS_ID
        ys, xs = np.mgrid[0:H, 0:W]
        loads = {"none_below": np.full((H, W), 8.0, np.float32), "camera_move": moved[..., 3].copy(), "all_below": np.full((H, W), 1.0, np.float32),
                 "checkerboard": np.where((xs + ys) % 2 == 0, 1.0, 8.0).astype(np.float32)}
        d = T.Reconstruct(); dr = T.Rectify()
        reconstruct = lambda: pt._check(pt._L.idkptReconstructHistory(pt._ctx, 1, C.addressof(d)))   # noqa: E731
        reproject = lambda: pt._check(pt._L.idkptReproject(pt._ctx, 1, 0, C.addressof(s)))            # noqa: E731
        rectify = lambda: pt._check(pt._L.idkptRectifyHistory(pt._ctx, 1, C.addressof(dr)))           # noqa: E731
        row = {"size": [W, H], "hit_pixels": round(float(hit.mean()), 4), "share_below_fill_below_of_hit_pixels": {}, "pixels_changed_by_the_first_call": {}}
        names = [f"ms_reconstruct_{k}" for k in loads] + ["ms_reproject", "ms_rectify_radius_2"]
        for name in names:
            row[name] = []
        for _ in range(3):                                                                          # three rounds, the calls alternating
            for k, alpha in loads.items():
                img = moved.copy(); img[..., 3] = alpha
                write_temporal(img)
                if not row[f"ms_reconstruct_{k}"]:
                    row["share_below_fill_below_of_hit_pixels"][k] = round(float((hit & (alpha < fill)).sum() / max(1, hit.sum())), 4)
                    reconstruct()
                    row["pixels_changed_by_the_first_call"][k] = round(float((R.bits(pt.DownloadTemporal(1)) != R.bits(img)).any(axis=2).mean()), 4)
                row[f"ms_reconstruct_{k}"].append(timed(reconstruct))
            row["ms_reproject"].append(timed(reproject))                                            # (rewrites the temporal image of slot 1: the next round plants it again)
            row["ms_rectify_radius_2"].append(timed(rectify))
        print(json.dumps(row), flush=True)
        res["time"].append(row)
        pt.Dispose()

    # ---- quality
    QW = QH = 64

    def cam(t):                                                                                     # the move of profiles/reproject.md
        return S.Camera(QW, QH, position=(0.02 * t, 0.0, 3.4), view_dir=(np.sin(np.radians(0.4 * t)), 0.0, -np.cos(np.radians(0.4 * t))), fovy_deg=40.0)

    def truth(t):
        ref = PathTracer(QW, QH); ref.RayDepth = 4; ref.UploadScene(box); ref.SetCamera(cam(t)); ref.set_max_batch(32)
        for _ in range(args.reference_samples):
            ref.Compute()
        img = ref.Result[..., :3].astype(np.float64); ref.Dispose()
        return img

    def context():
        pt = PathTracer(QW, QH); pt.RayDepth = 4; pt.OutputAOVs = 1; pt.UploadScene(box); pt.SetFrameRing(2); pt.SetNoiseEstimate(True)
        return pt

    def rmse(img, ref, mask):
        if not mask.any():
            return None
        return round(float(np.sqrt(np.mean((img[..., :3].astype(np.float64)[mask] - ref[mask]) ** 2))), 5)

    judged = {8: "+0", 9: "+1", 10: "+2", 12: "+4"}
    with_c, without = context(), context()
    q = {"reference_samples": args.reference_samples, "columns": "[with reconstruction, without]", "frames": {}}
    prev, prev_cam = T.IDKPT_NO_HISTORY, None
    everything = np.ones((QH, QW), bool)
    mask8 = None
    for k in range(13):
        s = T.Reproject() if prev_cam is None else T.Reproject.from_camera(prev_cam)
        sf = T.Reproject(MaxHistory=4.0) if prev_cam is None else T.Reproject.from_camera(prev_cam, MaxHistory=4.0)
        for pt in (with_c, without):
            pt.SetSampleSequence(k, 1)
            slot = pt.BeginFrame(); pt.SetCamera(cam(k)); pt.Compute(); pt.CaptureGeometry()
            pt.Reproject(slot, prev, s); pt.ReprojectMoments(slot, prev, s); pt.ReprojectFast(slot, prev, sf)
        before = with_c.DownloadTemporal(slot)
        with_c.ReconstructHistory(slot)
        if k in judged:
            ref = truth(k)
            imgs = [with_c.DownloadTemporal(slot), without.DownloadTemporal(slot)]
            den = [with_c.DenoiseTemporal(slot=slot), without.DenoiseTemporal(slot=slot)]
            hit = R.bits(with_c.DownloadGeometry(slot)[..., 3]) != R.MISS_ID
            below = hit & (before[..., 3] < fill)
            below_without = hit & (imgs[1][..., 3] < fill)
            if k == 8:
                mask8 = below
            rec = {"frame": k, "hit_pixels": int(hit.sum()), "pixels_below_fill_below": [int(below.sum()), int(below_without.sum())],
                   "pixels_changed": int((R.bits(imgs[0]) != R.bits(before)).any(axis=2).sum()),
                   "rmse_temporal_below": [rmse(imgs[0], ref, below), rmse(imgs[1], ref, below)], "rmse_temporal_all": [rmse(imgs[0], ref, everything), rmse(imgs[1], ref, everything)],
                   "rmse_denoise_temporal_below": [rmse(den[0], ref, below), rmse(den[1], ref, below)], "rmse_denoise_temporal_all": [rmse(den[0], ref, everything), rmse(den[1], ref, everything)],
                   "rmse_temporal_on_frame_8s_pixels": [rmse(imgs[0], ref, mask8), rmse(imgs[1], ref, mask8)],
                   "rmse_denoise_temporal_on_frame_8s_pixels": [rmse(den[0], ref, mask8), rmse(den[1], ref, mask8)]}
            q["frames"][judged[k]] = rec
            print(json.dumps({judged[k]: rec}), flush=True)
        prev, prev_cam = slot, cam(k)
    with_c.Dispose(); without.Dispose()
    res["quality"]["cornell_camera_move"] = q
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
