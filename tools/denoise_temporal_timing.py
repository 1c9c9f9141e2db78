"""What the temporal moments cost and give (profiles/denoise_temporal.md).  Needs a GPU; prints one JSON object and writes it to --out.

Times, by HIP events around --reps calls after 3 warm-up calls, at 1920 x 1080 and 3840 x 2160 in one run: idkptReprojectMoments beside idkptReproject over two captures
of the Cornell box under two cameras; idkptDenoiseTemporal beside idkptDenoiseVariance with Iterations 1 .. 6 (DemodulateAlbedo 0) and with the defaults, alternating.
The filters read tests/denoise_temporal_ref.py's seeded images, tiled (counts on both sides of SpatialBelow).  The pre-pass k_temporal_state is reported as the whole call
with Iterations = 1 minus idkptDenoiseVariance's with Iterations = 1 (whose one launch also makes its first state: the difference is the pre-pass's launch), with the
planted counts, with every count at 33 (no pixel walks the 49 taps) and with every count at 1 (every pixel does).

Quality: the 64 x 64 Cornell box, one sample per frame along a small camera move, frames 0 .. 7 the history and frame 8 the one judged against --reference-samples
samples from frame 8's camera: RMSE of the one-sample frame, of the temporal image (idkptUseTemporalAsDenoised), of idkptDenoise under the temporal input and of
idkptDenoiseTemporal, all with their defaults (nothing is swept here)."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reference-samples", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("denoise_temporal_timing needs a GPU")
    from idkengine_amd import _lib, gputypes as T, scenes as S
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    import denoise_temporal_ref as R
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    box = S.cornell_scene(NativeBuilder(), variant="mixed")
    res = {"reps": args.reps, "time": [], "quality": {}}

    for W, H in ((1920, 1080), (3840, 2160)):
        pt = PathTracer(W, H)
        pt.RayDepth = 2; pt.OutputAOVs = 1
        pt.UploadScene(box); pt.SetFrameRing(2); pt.SetNoiseEstimate(True)
        st = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(st)))
        stream = torch.cuda.ExternalStream(st.value)
        cam_a = S.Camera(W, H, position=(0.0, 0.0, 3.4), view_dir=(0.0, 0.0, -1.0), fovy_deg=40.0)
        cam_b = S.Camera(W, H, position=(0.02, 0.0, 3.4), view_dir=(0.01, 0.0, -1.0), fovy_deg=40.0)
        pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute(); pt.Compute(); pt.CaptureGeometry(); pt.Reproject(0, T.IDKPT_NO_HISTORY); pt.ReprojectMoments(0, T.IDKPT_NO_HISTORY)
        pt.BeginFrame(); pt.SetCamera(cam_b); pt.Compute(); pt.Compute(); pt.CaptureGeometry(); pt.synchronize()
        s = T.Reproject.from_camera(cam_a)

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

        reproject = lambda: pt._check(pt._L.idkptReproject(pt._ctx, 1, 0, C.addressof(s)))                   # noqa: E731
        reproject_moments = lambda: pt._check(pt._L.idkptReprojectMoments(pt._ctx, 1, 0, C.addressof(s)))   # noqa: E731
        row = {"size": [W, H]}
        row["ms_reproject"] = [timed(reproject) for _ in range(3)]
        row["ms_reproject_moments"] = [timed(reproject_moments) for _ in range(3)]
        row["history_fraction"] = round(float((pt.DownloadTemporalMoments(1)[..., 3] > 2.0).mean()), 4)

        # the filters on planted images: slot 1 holds two samples (idkptDenoiseVariance's N), a temporal image and a temporal moments image
        tile = R.random_images(240, 135)
        moments_tile = tile[1].copy(); moments_tile[..., 3] = 1.0
        ptrs = [pt.temporal_device_ptr(1)[0], pt.temporal_moments_device_ptr(1)[0], pt.frame_device_ptr(1, 1)[0], pt.frame_device_ptr(1, 2)[0], pt.frame_device_ptr(1, 0)[0], pt.moments_device_ptr(1)[0]]

        def plant(p, im):
            holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (H, W, 4), "typestr": "<f4", "data": (int(p), False), "version": 2}})()
            with torch.cuda.stream(stream):
                torch.as_tensor(holder, device="cuda").copy_(torch.from_numpy(np.tile(im, (H // 135, W // 240, 1))).to("cuda"))
            stream.synchronize()

        for p, im in zip(ptrs, list(tile) + [tile[0], moments_tile]):
            plant(p, im)

        def variance(it, demod):
            d = T.DenoiseVariance(Iterations=it, DemodulateAlbedo=demod)
            return lambda: pt._check(pt._L.idkptDenoiseVariance(pt._ctx, 1, C.addressof(d)))

        def temporal(it, demod):
            d = T.DenoiseTemporal(Iterations=it, DemodulateAlbedo=demod)
            return lambda: pt._check(pt._L.idkptDenoiseTemporal(pt._ctx, 1, C.addressof(d)))

        rounds = [(timed(variance(5, 1)), timed(temporal(5, 1))) for _ in range(3)]
        row["ms_default_call_denoise_variance"] = [a for a, _ in rounds]; row["ms_default_call_denoise_temporal"] = [b for _, b in rounds]
        row["ms_denoise_variance_iterations_1_to_6"] = [timed(variance(k, 0)) for k in range(1, 7)]
        row["ms_denoise_temporal_iterations_1_to_6"] = [timed(temporal(k, 0)) for k in range(1, 7)]
        row["spatial_fraction_planted"] = round(float((tile[1][..., 3] < 4.0).mean()), 4)
        row["ms_prepass_planted_counts"] = round(row["ms_denoise_temporal_iterations_1_to_6"][0] - row["ms_denoise_variance_iterations_1_to_6"][0], 4)
        for name, cnt in (("ms_prepass_no_pixel_spatial", 33.0), ("ms_prepass_every_pixel_spatial", 1.0)):
            tm = tile[1].copy(); tm[..., 3] = cnt
            plant(ptrs[1], tm)
            row[name] = round(timed(temporal(1, 0)) - row["ms_denoise_variance_iterations_1_to_6"][0], 4)
        v, t = row["ms_denoise_variance_iterations_1_to_6"], row["ms_denoise_temporal_iterations_1_to_6"]
        row["ms_tiled_iteration_spacing_2_and_4"] = [round(v[1] - v[0], 4), round(v[2] - v[1], 4), round(t[1] - t[0], 4), round(t[2] - t[1], 4)]
        print(json.dumps(row), flush=True)
        res["time"].append(row)
        pt.Dispose()

    # ---- quality on the small Cornell box
    w = h = 64

    def cam(k):                                                                                  # the move of tools/reproject_timing.py: 0.02 along x and 0.4 degrees of yaw per frame
        return S.Camera(w, h, position=(0.02 * k, 0.0, 3.4), view_dir=(np.sin(np.radians(0.4 * k)), 0.0, -np.cos(np.radians(0.4 * k))), fovy_deg=40.0)

    ref = PathTracer(w, h); ref.RayDepth = 4; ref.UploadScene(box); ref.SetCamera(cam(8)); ref.set_max_batch(32)
    for _ in range(args.reference_samples):
        ref.Compute()
    truth = ref.Result[..., :3].astype(np.float64); ref.Dispose()
    rmse = lambda img: round(float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - truth) ** 2))), 5)   # noqa: E731
    pt = PathTracer(w, h); pt.RayDepth = 4; pt.OutputAOVs = 1; pt.UploadScene(box); pt.SetFrameRing(2); pt.SetNoiseEstimate(True)
    prev_cam, prev = None, T.IDKPT_NO_HISTORY
    for k in range(9):                                                                           # frames 0..7 are the history, frame 8 is the one that is judged
        slot = pt.BeginFrame(); pt.SetCamera(cam(k)); pt.Compute(); pt.CaptureGeometry()
        s = T.Reproject.from_camera(prev_cam) if prev_cam is not None else None
        pt.Reproject(slot, prev, s); pt.ReprojectMoments(slot, prev, s)
        prev_cam, prev = cam(k), slot
    q = res["quality"]
    q["reference_samples"] = args.reference_samples
    q["rmse_1_sample"] = rmse(pt.FrameResult(prev))
    pt.UseTemporalAsDenoised(prev); q["rmse_use_temporal_as_denoised"] = rmse(pt.DownloadDenoised(prev))
    pt.SetDenoiseInput(T.IDKPT_DENOISE_INPUT_TEMPORAL); q["rmse_denoise_on_temporal_input"] = rmse(pt.Denoise(slot=prev)); pt.SetDenoiseInput(T.IDKPT_DENOISE_INPUT_ACCUMULATED)
    q["rmse_denoise_temporal"] = rmse(pt.DenoiseTemporal(slot=prev))
    tm = pt.DownloadTemporalMoments(prev)
    q["mean_effective_samples"] = round(float(tm[..., 3].mean()), 3); q["pixels_below_spatial_below"] = round(float((tm[..., 3] < 4.0).mean()), 4)
    pt.Dispose()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
