"""What history rectification costs and gives (profiles/rectify.md).  Needs a GPU; prints one JSON object and writes it to --out.

Times, by HIP events around --reps calls after 3 warm-up calls, at 1920 x 1080 and 3840 x 2160 in one run, three rounds that alternate the calls: idkptRectifyHistory
(Radius 2; one launch of k_rectify, with the temporal moments image) beside idkptReproject and idkptReprojectFast over two captures of the Cornell box, and beside
k_temporal_state, reported as tools/denoise_temporal_timing.py reports it: idkptDenoiseTemporal with Iterations = 1 minus idkptDenoiseVariance with Iterations = 1.
Radius 1 and 3 once each.  The fast history of the timed slot is the long one plus a planted change on half of the frame, so that both branches of the kernel run.

Quality: a static camera, one sample per frame (frame k draws the random numbers of sample k: idkptSetSampleSequence), --history frames, then a change of lighting, then 16 more frames; two contexts run the same frames, one with
idkptReprojectFast + idkptRectifyHistory and one without.  RMSE against --reference-samples samples of the NEW lighting at +2, +4, +8 and +16 frames, of the temporal image
and behind idkptDenoiseTemporal; on the 8 frames before the change, RMSE against as many samples of the OLD lighting and the share of pixels the rectification moved.
Scenes: the 64 x 64 Cornell box of profiles/reproject.md with the light's emission x 4 (idkptUpdateBuffer of the materials), and an open triangle soup under a uniform
sky x 3 (idkptUpdateSky).  Radius, ZLow, ZHigh, Epsilon and the fast cap are the documented starting values: nothing is swept here."""
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
    ap.add_argument("--history", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rectify_timing needs a GPU")
    from idkengine_amd import _lib, gputypes as T, scenes as S
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    import rectify_ref as R
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    builder = NativeBuilder()
    box = S.cornell_scene(builder, variant="mixed")
    res = {"reps": args.reps, "time": [], "quality": {}}

    for W, H in ((1920, 1080), (3840, 2160)):
        pt = PathTracer(W, H)
        pt.RayDepth = 2; pt.OutputAOVs = 1
        pt.UploadScene(box); pt.SetFrameRing(2); pt.SetNoiseEstimate(True)
        st = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(st)))
        stream = torch.cuda.ExternalStream(st.value)
        cam_a = S.Camera(W, H, position=(0.0, 0.0, 3.4), view_dir=(0.0, 0.0, -1.0), fovy_deg=40.0)
        cam_b = S.Camera(W, H, position=(0.02, 0.0, 3.4), view_dir=(0.01, 0.0, -1.0), fovy_deg=40.0)
        pt.BeginFrame(); pt.SetCamera(cam_a); pt.Compute(); pt.Compute(); pt.CaptureGeometry()
        pt.Reproject(0, T.IDKPT_NO_HISTORY); pt.ReprojectMoments(0, T.IDKPT_NO_HISTORY); pt.ReprojectFast(0, T.IDKPT_NO_HISTORY)
        pt.BeginFrame(); pt.SetCamera(cam_b); pt.Compute(); pt.Compute(); pt.CaptureGeometry(); pt.synchronize()
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

        # the fast history: the long one, brighter by a fifth on the right half of the frame (every call rereads it; the long one converges towards it there)
        f = pt.DownloadTemporal(1); f[:, W // 2:, :3] *= np.float32(1.2); f[..., 3] = 4.0
        holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (H, W, 4), "typestr": "<f4", "data": (int(pt.fast_temporal_device_ptr(1)[0]), False), "version": 2}})()
        with torch.cuda.stream(stream):
            torch.as_tensor(holder, device="cuda").copy_(torch.from_numpy(f).to("cuda"))
        stream.synchronize()
        before = pt.DownloadTemporal(1)
        pt.RectifyHistory(slot=1)
        row = {"size": [W, H], "pixels_moved_by_the_first_call": round(float((R.bits(pt.DownloadTemporal(1)) != R.bits(before)).any(axis=2).mean()), 4)}

        def rectify(radius):
            d = T.Rectify(Radius=radius)
            return lambda: pt._check(pt._L.idkptRectifyHistory(pt._ctx, 1, C.addressof(d)))

        def variance1():
            d = T.DenoiseVariance(Iterations=1, DemodulateAlbedo=0)
            return lambda: pt._check(pt._L.idkptDenoiseVariance(pt._ctx, 1, C.addressof(d)))

        def temporal1():
            d = T.DenoiseTemporal(Iterations=1, DemodulateAlbedo=0)
            return lambda: pt._check(pt._L.idkptDenoiseTemporal(pt._ctx, 1, C.addressof(d)))

        reproject = lambda: pt._check(pt._L.idkptReproject(pt._ctx, 1, 0, C.addressof(s)))            # noqa: E731
        reproject_fast = lambda: pt._check(pt._L.idkptReprojectFast(pt._ctx, 1, 0, C.addressof(sf)))  # noqa: E731
        calls = [("ms_rectify_radius_2", rectify(2)), ("ms_reproject", reproject), ("ms_denoise_variance_1_iteration", variance1()), ("ms_denoise_temporal_1_iteration", temporal1())]
        for name, _ in calls:
            row[name] = []
        for _ in range(3):                                                                          # three rounds, the calls alternating
            for name, fn in calls:
                row[name].append(timed(fn))
        row["ms_k_temporal_state"] = [round(a - b, 4) for a, b in zip(row["ms_denoise_temporal_1_iteration"], row["ms_denoise_variance_1_iteration"])]
        row["ms_rectify_radius_1"] = timed(rectify(1)); row["ms_rectify_radius_3"] = timed(rectify(3))
        row["ms_reproject_fast"] = timed(reproject_fast)
        print(json.dumps(row), flush=True)
        res["time"].append(row)
        pt.Dispose()

    # ---- quality
    QW = QH = 64
    def run_quality(name, scene, cam, depth, change):
        def context():
            pt = PathTracer(QW, QH); pt.RayDepth = depth; pt.OutputAOVs = 1; pt.UploadScene(scene); pt.SetFrameRing(2); pt.SetNoiseEstimate(True)
            return pt

        def truth(changed):
            ref = PathTracer(QW, QH); ref.RayDepth = depth; ref.UploadScene(scene)
            if changed:
                change(ref)
            ref.SetCamera(cam); ref.set_max_batch(32)
            for _ in range(args.reference_samples):
                ref.Compute()
            img = ref.Result[..., :3].astype(np.float64); ref.Dispose()
            return img

        old_truth, new_truth = truth(False), truth(True)
        rmse = lambda img, ref: round(float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref) ** 2))), 5)   # noqa: E731
        with_r, without = context(), context()
        long_s, fast_s = T.Reproject.from_camera(cam), T.Reproject.from_camera(cam, MaxHistory=4.0)
        q = {"reference_samples": args.reference_samples, "history_frames": args.history, "steady": [], "after": {}}
        prev = T.IDKPT_NO_HISTORY
        for k in range(args.history + 16):
            if k == args.history:
                change(with_r); change(without)
            for pt in (with_r, without):
                pt.SetSampleSequence(k, 1)                                                        # frame k draws sample k's random numbers: a static camera would otherwise render the same noise every frame
                slot = pt.BeginFrame(); pt.SetCamera(cam); pt.Compute(); pt.CaptureGeometry()
                pt.Reproject(slot, prev, long_s); pt.ReprojectMoments(slot, prev, long_s)
            with_r.ReprojectFast(slot, prev, fast_s)
            before = with_r.DownloadTemporal(slot)
            with_r.RectifyHistory(slot=slot)
            moved = float((R.bits(with_r.DownloadTemporal(slot)) != R.bits(before)).any(axis=2).mean())
            after = k - args.history + 1                                                            # the frame that first sees the change is +1
            ref = new_truth if after >= 1 else old_truth
            rec = {"frame": k, "pixels_moved": round(moved, 4),
                   "rmse_temporal": [rmse(with_r.DownloadTemporal(slot), ref), rmse(without.DownloadTemporal(slot), ref)],
                   "rmse_denoise_temporal": [rmse(with_r.DenoiseTemporal(slot=slot), ref), rmse(without.DenoiseTemporal(slot=slot), ref)],
                   "mean_effective_samples": [round(float(with_r.DownloadTemporal(slot)[..., 3].mean()), 3), round(float(without.DownloadTemporal(slot)[..., 3].mean()), 3)]}
            if after in (2, 4, 8, 16):
                q["after"][f"+{after}"] = rec
            elif -8 < after <= 0:
                q["steady"].append(rec)
            prev = slot
        q["steady_mean"] = {key: [round(float(np.mean([r[key][i] for r in q["steady"]])), 5) for i in (0, 1)] for key in ("rmse_temporal", "rmse_denoise_temporal")}
        q["steady_mean"]["pixels_moved"] = round(float(np.mean([r["pixels_moved"] for r in q["steady"]])), 4)
        q["columns"] = "[with rectification, without]"
        with_r.Dispose(); without.Dispose()
        print(json.dumps({name: q}), flush=True)
        res["quality"][name] = q

    def brighter_light(pt):
        m = box.materials.copy(); m["EmissiveFactor"] *= np.float32(4.0)
        pt.UpdateBuffer(T.IDKPT_BUF_MATERIALS, m)

    run_quality("cornell_emission_x4", box, S.Camera(QW, QH, position=(0.0, 0.0, 3.4), view_dir=(0.0, 0.0, -1.0), fovy_deg=40.0), 4, brighter_light)
    soup = S.presplit_scene(builder)

    def brighter_sky(pt):
        faces = soup.sky_faces.copy(); faces[..., :3] *= np.float32(3.0)
        pt.UpdateSky(np.ascontiguousarray(faces))

    run_quality("open_soup_sky_x3", soup, S.presplit_camera(QW, QH), 4, brighter_sky)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
