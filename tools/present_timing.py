"""What a displayed frame costs to leave the device: idkptDownload(Result) — 16 B per pixel — against idkptPresent + idkptDownloadDisplay — the tone-mapped RGBA8 image,
4 B per pixel — for the same frame on the same box (wall time, median of --reps runs), and k_present alone by HIP events on the context's stream for both formats, with
the bytes it moves (RGBA8: 16 B read + 4 B written per pixel; RGBA32F: 16 + 16).  The kernel's own line: run this under
`rocprofv3 --kernel-trace --stats -- python tools/present_timing.py` and read k_present.  Results: profiles/present.md.

Usage: python tools/present_timing.py [--width 1920] [--height 1080] [--reps 9] [--warmup 3]"""
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
    return f"median {np.median(ts):9.4f} ms  min {ts.min():9.4f}  max {ts.max():9.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080); ap.add_argument("--reps", type=int, default=9); ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch  # (one HIP runtime per process: torch's first)
    from idkengine_amd import gputypes as T, _lib
    from idkengine_amd.pathtracer import PathTracer
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    w, h = a.width, a.height
    pt = PathTracer(w, h)
    stream = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(stream)))
    ext = torch.cuda.ExternalStream(stream.value)
    # a frame with content: random radiance written into the result image (no scene is needed to present)
    ptr, nbytes = pt.image_device_ptr(0)
    holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (h, w, 4), "typestr": "<f4", "data": (int(ptr), False), "version": 2}})()
    with torch.cuda.stream(ext):
        torch.as_tensor(holder, device="cuda").copy_(torch.rand((h, w, 4), device="cuda") * 3.0)
    ext.synchronize()
    tm = T.TonemapSettings()
    px = w * h
    for fmt, name, moved in ((T.IDKPT_DISPLAY_RGBA8, "RGBA8", 20 * px), (T.IDKPT_DISPLAY_RGBA32F, "RGBA32F", 32 * px)):
        ev = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext); pt._check(pt._L.idkptPresent(pt._ctx, -1, 0, C.addressof(tm), fmt, None, None)); e1.record(ext)
            pt.synchronize()
            if i >= a.warmup:
                ev.append(e0.elapsed_time(e1))
        print(f"k_present {name:8s} {w} x {h}: by HIP events {stats(ev)}  -> {moved / 1e6:.1f} MB moved, {moved / (np.median(ev) * 1e-3) / 1e9:.0f} GB/s at the median", flush=True)
    full = np.zeros((h, w, 4), np.float32); disp = np.zeros((h, w, 4), np.uint8)
    t_full, t_disp = [], []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter(); pt._check(pt._L.idkptDownload(pt._ctx, 0, full.ctypes.data, full.nbytes)); t1 = time.perf_counter()
        pt._check(pt._L.idkptPresent(pt._ctx, -1, 0, C.addressof(tm), T.IDKPT_DISPLAY_RGBA8, None, None)); pt._check(pt._L.idkptDownloadDisplay(pt._ctx, -1, disp.ctypes.data, disp.nbytes)); t2 = time.perf_counter()
        if i >= a.warmup:
            t_full.append((t1 - t0) * 1e3); t_disp.append((t2 - t1) * 1e3)
    print(f"idkptDownload(Result)               {full.nbytes / 1e6:6.1f} MB: {stats(t_full)}", flush=True)
    print(f"idkptPresent + idkptDownloadDisplay {disp.nbytes / 1e6:6.1f} MB: {stats(t_disp)}", flush=True)
    print(f"ratio of the medians: {np.median(t_full) / np.median(t_disp):.2f}x  ({a.reps} runs after {a.warmup} warm; pageable host memory on both sides)", flush=True)
    assert disp[..., 3].min() == 255 and disp[..., :3].max() > 0
    pt.Dispose()


if __name__ == "__main__":
    main()
