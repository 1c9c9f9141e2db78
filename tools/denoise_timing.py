"""Times idkptDenoise on the device (profiles/denoise.md): per call and per iteration at 1920 x 1080 and 3840 x 2160, against the compulsory-traffic model — 64 bytes per
pixel and iteration (48 read, 16 written) at the copy bandwidth measured in the same run.  Needs a GPU; prints one JSON line per size and writes them to --out.

Per-iteration times are differences of whole calls with Iterations = k and k - 1 (DemodulateAlbedo 0, so that iteration k - 1 does the same work in both): iteration i
uses tap spacing 1 << i; spacings 1, 2, 4 run k_denoise_tile, 8 and up k_denoise_direct (idkptGetDenoiseRoute), so the series also compares the two routes on equal work."""
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
        sys.exit("denoise_timing needs a GPU")
    from idkengine_amd import _lib, gputypes as T
    from idkengine_amd.pathtracer import PathTracer
    import denoise_ref as R
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    lines = []
    for W, H in ((1920, 1080), (3840, 2160)):
        pt = PathTracer(W, H); pt.OutputAOVs = 1
        st = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(st)))
        stream = torch.cuda.ExternalStream(st.value)
        tile = R.random_images(240, 135)
        with torch.cuda.stream(stream):
            for i in range(3):
                p, n = pt.frame_device_ptr(0, i)
                holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (H, W, 4), "typestr": "<f4", "data": (int(p), False), "version": 2}})()
                torch.as_tensor(holder, device="cuda").copy_(torch.from_numpy(np.tile(tile[i], (H // 135, W // 240, 1))).to("cuda"))
            # the copy bandwidth of this run: a device-to-device copy of 3 images' worth (reads + writes counted)
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

        def call(it, demod):
            d = T.Denoise(Iterations=it, DemodulateAlbedo=demod)
            return lambda: pt._check(pt._L.idkptDenoise(pt._ctx, -1, C.addressof(d)))

        series = [timed(call(k, 0), args.reps) for k in range(1, 7)]
        per_iter = [series[0]] + [series[k] - series[k - 1] for k in range(1, 6)]
        default_ms = timed(call(5, 1), args.reps)
        routes = [pt.denoise_route(i) for i in range(5)]
        model_ms = 64.0 * W * H / copy_bw * 1e3
        line = dict(size=[W, H], reps=args.reps, copy_GBps=round(copy_bw / 1e9, 1), model_ms_per_iteration=round(model_ms, 4),
                    ms_per_iteration=[round(v, 4) for v in per_iter], routes_of_default_call=routes, ms_calls_iterations_1_to_6_no_demod=[round(v, 4) for v in series],
                    ms_default_call=round(default_ms, 4), default_call_over_model=round(default_ms / (5 * model_ms), 2))
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
