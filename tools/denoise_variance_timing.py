"""Times idkptDenoiseVariance beside idkptDenoise on the device (profiles/denoise_variance.md): the same frames at 1920 x 1080 and 3840 x 2160, the same 5 iterations,
the two calls alternating in one run, by HIP events around --reps calls after 3 warm-up calls.  Needs a GPU; prints one JSON line per size and writes them to --out.

The context renders two samples of the Cornell box with the noise switch and OutputAOVs on (the filter needs an accumulated count of 2), then Result, Albedo, Normal and
the moments are overwritten with tests/denoise_variance_ref.py's seeded images, tiled.  Per-iteration times are differences of whole calls with Iterations = k and k - 1
(DemodulateAlbedo 0): iteration i uses tap spacing 1 << i; spacings 1, 2, 4 run the tiled kernels, 8 and up the direct ones (idkptGetDenoiseRoute).  The first
iteration of idkptDenoiseVariance also reads the moments (16 B per pixel more)."""
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("denoise_variance_timing needs a GPU")
    from idkengine_amd import _lib, gputypes as T, scenes as S
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    import denoise_variance_ref as R
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    sc = S.cornell_scene(NativeBuilder(), variant="mixed")
    lines = []
    for W, H in ((1920, 1080), (3840, 2160)):
        pt = PathTracer(W, H)
        pt.UploadScene(sc); pt.SetCamera(S.cornell_camera(W, H)); pt.RayDepth = 2; pt.OutputAOVs = 1
        pt.SetNoiseEstimate(True)
        pt.Compute(); pt.Compute()
        assert pt.AccumulatedSamples == R.SAMPLES
        st = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(st)))
        stream = torch.cuda.ExternalStream(st.value)
        tile = R.random_images(240, 135)
        ptrs = [pt.frame_device_ptr(0, i)[0] for i in range(3)] + [pt.moments_device_ptr()[0]]
        with torch.cuda.stream(stream):
            for p, im in zip(ptrs, tile):
                holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (H, W, 4), "typestr": "<f4", "data": (int(p), False), "version": 2}})()
                torch.as_tensor(holder, device="cuda").copy_(torch.from_numpy(np.tile(im, (H // 135, W // 240, 1))).to("cuda"))
            src = torch.empty(H * W * 12, dtype=torch.float32, device="cuda"); dst = torch.empty_like(src)
        stream.synchronize()

        def timed(fn, reps):
            with torch.cuda.stream(stream):
                for _ in range(3):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    fn()
                e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

        copy_ms = timed(lambda: dst.copy_(src), args.reps)
        copy_bw = 2.0 * src.numel() * 4 / (copy_ms * 1e-3)

        def plain(it, demod):
            d = T.Denoise(Iterations=it, DemodulateAlbedo=demod)
            return lambda: pt._check(pt._L.idkptDenoise(pt._ctx, -1, C.addressof(d)))

        def variance(it, demod):
            d = T.DenoiseVariance(Iterations=it, DemodulateAlbedo=demod)
            return lambda: pt._check(pt._L.idkptDenoiseVariance(pt._ctx, -1, C.addressof(d)))

        # the default calls, alternating, three rounds: the spread between rounds is the noise of the run
        rounds = [(timed(plain(5, 1), args.reps), timed(variance(5, 1), args.reps)) for _ in range(3)]
        routes = [pt.denoise_route(i) for i in range(5)]
        series_v = [timed(variance(k, 0), args.reps) for k in range(1, 7)]
        series_p = [timed(plain(k, 0), args.reps) for k in range(1, 7)]
        diff = lambda s: [s[0]] + [s[k] - s[k - 1] for k in range(1, 6)]   # noqa: E731
        line = dict(size=[W, H], reps=args.reps, copy_GBps=round(copy_bw / 1e9, 1), model_ms_per_iteration=round(64.0 * W * H / copy_bw * 1e3, 4),
                    ms_default_call_denoise=[round(a, 4) for a, _ in rounds], ms_default_call_denoise_variance=[round(b, 4) for _, b in rounds],
                    routes_of_default_call=routes, ms_per_iteration_denoise_variance=[round(v, 4) for v in diff(series_v)], ms_per_iteration_denoise=[round(v, 4) for v in diff(series_p)])
        print(json.dumps(line), flush=True)
        lines.append(line)
        pt.Dispose()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
