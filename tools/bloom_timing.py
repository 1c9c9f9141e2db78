"""What bloom costs on the device: idkptBloom (the whole chain: 2 * levels launches) by HIP events on the context's stream at 1080p and 4K, idkptBloom + idkptPresent
against idkptPresent alone, and what the host path it replaces moves (idkptDownload of Result, 16 B per pixel, and the upload of a full-size RGBA32F bloom image, 16 B
per pixel — timed here as the two copies alone, without the host's filter).  Per-pass times: run this under `rocprofv3 --kernel-trace -d DIR -o bloom --output-format csv
-- python tools/bloom_timing.py` and then `python tools/bloom_timing.py --summarize DIR/.../bloom_kernel_trace.csv`: the dispatches of k_bloom_* are grouped by their
position in the chain (k_bloom_down0 starts one).  Results: profiles/bloom.md.

Usage: python tools/bloom_timing.py [--sizes 1920x1080,3840x2160] [--reps 9] [--warmup 3] | --summarize kernel_trace.csv"""
import argparse
import csv
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


def compulsory_bytes(w, h, minus_lods=3):
    """bytes every pass must move once: its sources read once, its level written once (16 B image texels, 8 B level texels)"""
    w0, h0 = w // 2, h // 2
    levels = max(int(np.floor(np.log2(max(w0, h0)))) + 1 - minus_lods, 2)
    t = [max(w0 >> l, 1) * max(h0 >> l, 1) for l in range(levels)]
    down = 16 * w * h + 8 * t[0] + sum(8 * t[l - 1] + 8 * t[l] for l in range(1, levels))
    up = sum(8 * t[l + 1] * 2 + 8 * t[l] for l in range(levels - 1))
    expand = 8 * t[0] + 16 * w * h
    return levels, down, up, expand


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    name = lambda r: r["Kernel_Name"]
    rows = sorted((r for r in rows if "k_bloom" in name(r)), key=lambda r: int(r["Start_Timestamp"]))
    chains, cur = [], None
    for r in rows:
        if "k_bloom_down0" in name(r):
            cur = []; chains.append(cur)
        if cur is not None:
            cur.append(r)
    by_len = {}
    for ch in chains:
        by_len.setdefault(len(ch), []).append(ch)
    for n, group in sorted(by_len.items()):
        print(f"chains of {n} launches ({n // 2} levels): {len(group)} recorded")
        for k in range(n):
            us = np.array([(int(ch[k]["End_Timestamp"]) - int(ch[k]["Start_Timestamp"])) / 1e3 for ch in group])
            short = name(group[0][k]).split("(")[0]
            print(f"  launch {k:2d} {short:28s} grid {group[0][k].get('Grid_Size_X', group[0][k].get('Grid_Size', '?')):>8s}: median {np.median(us):8.2f} us  min {us.min():8.2f}  max {us.max():8.2f}")
        tot = np.array([sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in ch) / 1e3 for ch in group])
        span = np.array([(int(ch[-1]["End_Timestamp"]) - int(ch[0]["Start_Timestamp"])) / 1e3 for ch in group])
        print(f"  sum of the kernels: median {np.median(tot):8.2f} us; first start to last end: median {np.median(span):8.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160"); ap.add_argument("--reps", type=int, default=9); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import torch  # (one HIP runtime per process: torch's first)
    from idkengine_amd import gputypes as T, _lib
    from idkengine_amd.pathtracer import PathTracer
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        pt = PathTracer(w, h)
        stream = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(stream)))
        ext = torch.cuda.ExternalStream(stream.value)
        ptr, nbytes = pt.image_device_ptr(0)
        holder = type("DevArray", (), {"__cuda_array_interface__": {"shape": (h, w, 4), "typestr": "<f4", "data": (int(ptr), False), "version": 2}})()
        with torch.cuda.stream(ext):
            torch.as_tensor(holder, device="cuda").copy_(torch.rand((h, w, 4), device="cuda") * 6.0)
        ext.synchronize()
        bs, tm = T.BloomSettings(), T.TonemapSettings()
        levels, down, up, expand = compulsory_bytes(w, h)
        bloom_ptr = C.c_void_p(); n = C.c_size_t()

        def bloom():
            pt._check(pt._L.idkptBloom(pt._ctx, -1, 0, C.addressof(bs)))

        def present(add0):
            pt._check(pt._L.idkptPresent(pt._ctx, -1, 0, C.addressof(tm), T.IDKPT_DISPLAY_RGBA8, add0, None))

        def timed(fn):
            ev = []
            for i in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ext); fn(); e1.record(ext)
                pt.synchronize()
                if i >= a.warmup:
                    ev.append(e0.elapsed_time(e1))
            return ev

        t_bloom = timed(bloom)
        pt._check(pt._L.idkptGetBloomDevicePtr(pt._ctx, -1, C.byref(bloom_ptr), C.byref(n)))
        t_present = timed(lambda: present(None))
        t_both = timed(lambda: (bloom(), present(bloom_ptr.value)))
        moved = down + up + expand
        print(f"{w} x {h}: {levels} levels, {2 * levels} launches; compulsory bytes {moved / 1e6:.1f} MB (down {down / 1e6:.1f}, up {up / 1e6:.1f}, expand {expand / 1e6:.1f})", flush=True)
        print(f"  idkptBloom (whole chain + expand) by HIP events: {stats(t_bloom)}  -> {moved / (np.median(t_bloom) * 1e-3) / 1e9:.0f} GB/s of compulsory bytes at the median", flush=True)
        print(f"  idkptPresent alone (RGBA8)                      : {stats(t_present)}", flush=True)
        print(f"  idkptBloom + idkptPresent(dAdd0 = bloom)        : {stats(t_both)}", flush=True)
        # the replaced host path's traffic: Result down, a full-size RGBA32F bloom image up (pageable host memory), without the host's own filter
        full = np.zeros((h, w, 4), np.float32); dev = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        t_rt = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            pt._check(pt._L.idkptDownload(pt._ctx, 0, full.ctypes.data, full.nbytes))
            dev.copy_(torch.from_numpy(full)); torch.cuda.synchronize()
            if i >= a.warmup:
                t_rt.append((time.perf_counter() - t0) * 1e3)
        print(f"  host round trip it replaces ({2 * full.nbytes / 1e6:.0f} MB: 16 B/pixel down + 16 B/pixel up, copies only): {stats(t_rt)}", flush=True)
        pt.Dispose()


if __name__ == "__main__":
    main()
