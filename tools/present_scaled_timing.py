"""What the display chain costs when the render size is below the presentation size (idkptSetPresentationSize): idkptBloom and idkptPresent (RGBA8) writing a
--width x --height presentation image from render sizes of scale 1.0 (the unscaled kernels: k_bloom_down0 ... k_bloom_expand, k_present), 0.5 and 0.1 (k_present_scaled and
the scaled bloom), by HIP events on the context's stream (median, min, max of --reps runs after --warmup), and end to end for a host that wants the displayed frame:
idkptBloom + idkptPresent + idkptDownloadDisplay (4 B per presentation pixel) against idkptDownload(Result) (16 B per RENDER pixel: what a host had to fetch to scale,
bloom and tone-map on the CPU).  The kernels' own lines: run this under `rocprofv3 --kernel-trace --stats -- python tools/present_scaled_timing.py`, in a run of its
own.  Results: profiles/present_scaled.md.

A/B against an older build: IDKPT_LIB_PATH=<its libidkpt.so> python tools/present_scaled_timing.py --scales 1.0 (a library without idkptSetPresentationSize is never asked
for it at scale 1.0), in the same session as the run of this tree's library.

Usage: python tools/present_scaled_timing.py [--width 1920] [--height 1080] [--reps 15] [--warmup 3] [--scales 1.0,0.5,0.1]"""
import argparse
import ctypes as C
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    ts = np.array(ts)
    return f"median {np.median(ts):8.4f} ms  min {ts.min():8.4f}  max {ts.max():8.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080); ap.add_argument("--reps", type=int, default=15); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scales", default="1.0,0.5,0.1")
    a = ap.parse_args()
    import torch  # (one HIP runtime per process: torch's first)
    from idkengine_amd import gputypes as T, _lib
    from idkengine_amd.pathtracer import PathTracer
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    pw, ph = a.width, a.height
    tm, bs = T.TonemapSettings(), T.BloomSettings()
    for scale in (float(s) for s in a.scales.split(",")):
        w, h = int(pw * scale), int(ph * scale)                                   # Application.cs: renderRes = (int)(presentRes * RenderResolutionScale)
        pt = PathTracer(w, h)
        if (w, h) != (pw, ph):
            pt.SetPresentationSize(pw, ph)
        stream = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(stream)))
        ext = torch.cuda.ExternalStream(stream.value)
        ptr, nbytes = pt.image_device_ptr(0)
        holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (h, w, 4), "typestr": "<f4", "data": (int(ptr), False), "version": 2}})()
        with torch.cuda.stream(ext):
            torch.as_tensor(holder, device="cuda").copy_(torch.rand((h, w, 4), device="cuda") * 3.0)
        ext.synchronize()
        t_bloom, t_present, t_e2e, t_full = [], [], [], []
        disp = np.zeros((ph, pw, 4), np.uint8); full = np.zeros((h, w, 4), np.float32)
        add0 = C.c_void_p(); n = C.c_size_t()
        for i in range(a.warmup + a.reps):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            t0 = time.perf_counter()
            e0.record(ext); pt._check(pt._L.idkptBloom(pt._ctx, -1, 0, C.addressof(bs))); e1.record(ext)
            pt._check(pt._L.idkptGetBloomDevicePtr(pt._ctx, -1, C.byref(add0), C.byref(n)))
            pt._check(pt._L.idkptPresent(pt._ctx, -1, 0, C.addressof(tm), T.IDKPT_DISPLAY_RGBA8, add0, None)); e2.record(ext)
            pt._check(pt._L.idkptDownloadDisplay(pt._ctx, -1, disp.ctypes.data, disp.nbytes))
            t1 = time.perf_counter()
            pt._check(pt._L.idkptDownload(pt._ctx, 0, full.ctypes.data, full.nbytes))
            t2 = time.perf_counter()
            if i >= a.warmup:
                t_bloom.append(e0.elapsed_time(e1)); t_present.append(e1.elapsed_time(e2)); t_e2e.append((t1 - t0) * 1e3); t_full.append((t2 - t1) * 1e3)
        levels, w0, h0 = pt.bloom_info()
        print(f"scale {scale:.1f}: render {w} x {h} -> presentation {pw} x {ph}; bloom {levels} levels from {w0} x {h0}", flush=True)
        print(f"  idkptBloom   (HIP events)                          {stats(t_bloom)}", flush=True)
        print(f"  idkptPresent (HIP events, RGBA8, dAdd0 = bloom)    {stats(t_present)}   source {w * h * 16 / 1e6:.1f} MB, bloom {pw * ph * 16 / 1e6:.1f} MB read, {pw * ph * 4 / 1e6:.1f} MB written", flush=True)
        print(f"  bloom + present + idkptDownloadDisplay ({disp.nbytes / 1e6:5.1f} MB)  {stats(t_e2e)}   (wall)", flush=True)
        print(f"  idkptDownload(Result)                  ({full.nbytes / 1e6:5.1f} MB)  {stats(t_full)}   (wall; the host would still have to scale, bloom and tone-map)", flush=True)
        assert disp[..., 3].min() == 255 and disp[..., :3].max() > 0
        pt.Dispose()


if __name__ == "__main__":
    main()
