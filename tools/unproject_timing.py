"""What an HDR environment costs: idkptUnprojectSky (k_equirect_pack + k_sky_unproject, csrc/kernels_unproject.hpp) for a 2048 x 1024 and an 8192 x 4096 panorama — wall
time of the call, which synchronises —, beside the only route a host had before it: the same per-texel functions built for the host (tools/unproject_host_route.cpp,
16 threads) followed by idkptUpdateSky(RGBA32F) of the faces and a synchronisation.  Both routes must leave the same faces bit for bit wherever atan2f / asinf / powf of
the host's libm and the device's agree; the fraction of equal texels is printed.  The kernels' own lines: run this under
`rocprofv3 --kernel-trace --stats -- python tools/unproject_timing.py` and read k_equirect_pack / k_sky_unproject.  Results: profiles/sky_unproject.md.

Usage: python tools/unproject_timing.py [--reps 5] [--warmup 1] [--threads 16] [--sizes 2048x1024,8192x4096] [--channels 3]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))


def stats(ts):
    ts = np.array(ts)
    return f"median {np.median(ts):9.3f} ms  min {ts.min():9.3f}  max {ts.max():9.3f}"


def host_route():
    src, so = os.path.join(HERE, "unproject_host_route.cpp"), os.path.join(HERE, "unproject_host_route.so")
    hdr = os.path.join(ROOT, "idkengine_amd", "csrc", "unproject_texel.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared", src, "-o", so])
    L = C.CDLL(so)
    L.host_unproject.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]; L.host_unproject.restype = None
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=1); ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sizes", default="2048x1024,8192x4096"); ap.add_argument("--channels", type=int, default=3)
    a = ap.parse_args()
    host = host_route()
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from idkengine_amd import scenes as S, _lib
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    pt = PathTracer(64, 64); pt.UploadScene(S.cornell_scene(NativeBuilder())); pt.SetCamera(S.cornell_camera(64, 64))
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        n = W // 4
        rng = np.random.default_rng(W)
        img = (rng.random((H, W, a.channels), dtype=np.float32) ** 4 * 40.0).astype(np.float32)     # mostly dark, a few bright texels
        dev, cpu, up = [], [], []
        faces = np.empty((6, n, n, 4), np.float32)
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter(); pt.UnprojectSky(img); t1 = time.perf_counter()
            if i >= a.warmup:
                dev.append((t1 - t0) * 1e3)
        got = pt.DownloadSky()
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter(); host.host_unproject(img.ctypes.data, W, H, a.channels, n, faces.ctypes.data, a.threads); t1 = time.perf_counter()
            pt.UpdateSky(faces); pt.synchronize(); t2 = time.perf_counter()
            if i >= a.warmup:
                cpu.append((t1 - t0) * 1e3); up.append((t2 - t1) * 1e3)
        equal = float((got.view(np.uint32) == faces.view(np.uint32)).all(axis=-1).mean())
        steps = np.abs(got.astype(np.float16).view(np.uint16).astype(np.int64) - faces.astype(np.float16).view(np.uint16).astype(np.int64)).max()
        print(f"{W} x {H} x {a.channels} ({img.nbytes / 2**20:.0f} MiB) -> S = {n} ({faces.nbytes / 2**20:.0f} MiB of faces)", flush=True)
        print(f"    idkptUnprojectSky (upload, pack, unproject, synchronise): {stats(dev)}", flush=True)
        print(f"    host route: unprojection on {a.threads} threads {stats(cpu)};  idkptUpdateSky(RGBA32F) + idkptSynchronize {stats(up)};  together median {np.median(np.array(cpu) + np.array(up)):9.3f} ms", flush=True)
        print(f"    texels equal bit for bit between the routes: {equal:.6f}; largest distance {int(steps)} half step(s)  ({a.reps} runs after {a.warmup} warm)", flush=True)
    pt.ResetAccumulation(); pt.Compute(); assert np.isfinite(pt.Result).all()
    pt.Dispose()


if __name__ == "__main__":
    main()
