"""What the noise estimate costs on the device (profiles/noise.md): at 1920 x 1080 on the soup scene,
  * a batch of samples with idkptSetNoiseEstimate off and on, by HIP events around idkptRender + idkptFlush — the difference is what k_final_draw_noise adds to
    k_final_draw (32 B more per pixel read and written once per batch);
  * one idkptEstimateNoise (k_noise_estimate: 16 B per pixel read, 8 B per tile written), by HIP events, against the copy bandwidth measured in the same run.
Under rocprofv3 --kernel-trace --stats the lines of k_final_draw, k_final_draw_noise and k_noise_estimate give the kernels alone.

    python tools/noise_timing.py [--width 1920 --height 1080 --tris 100000 --batch 8 --reps 20]"""
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
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=100000); ap.add_argument("--batch", type=int, default=8); ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    w, h = a.width, a.height
    sc = S.soup_scene(a.tris, NativeBuilder(), seed=1)
    pt = PathTracer(w, h)
    pt.UploadScene(sc); pt.SetCamera(S.Camera(w, h)); pt.RayDepth = 2; pt.set_max_batch(a.batch)
    st = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(st)))
    stream = torch.cuda.ExternalStream(st.value)

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return float(np.median(out)), float(np.min(out)), float(np.max(out))

    def batch():
        for _ in range(a.batch):
            pt.Compute()
        pt.flush()

    res = {"width": w, "height": h, "batch": a.batch, "reps": a.reps}
    for on in (0, 1, 0, 1):                                # off, on, off, on: the second pair shows the run-to-run spread
        pt.SetNoiseEstimate(on)
        for _ in range(3):
            batch()
        res.setdefault("batch_ms_on" if on else "batch_ms_off", []).append(timed(batch, a.reps))
    p = T.Noise()
    est = lambda: pt._check(pt._L.idkptEstimateNoise(pt._ctx, -1, C.addressof(p)))   # noqa: E731
    for _ in range(3):
        est()
    res["estimate_ms"] = timed(est, a.reps)
    src = torch.empty(w * h * 4, dtype=torch.float32, device="cuda"); dst = torch.empty_like(src)
    with torch.cuda.stream(stream):
        cp = timed(lambda: dst.copy_(src), a.reps)
    res["copy_16B_per_pixel_ms"] = cp
    res["copy_GBps"] = 2 * src.numel() * 4 / (cp[0] * 1e-3) / 1e9
    tiles, s = pt.DownloadNoise()
    res["summary"] = {k: float(v) for k, v in s.items()}
    print(json.dumps(res))
    pt.Dispose()


if __name__ == "__main__":
    main()
