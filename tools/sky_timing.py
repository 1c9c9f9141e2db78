"""What a sun move costs: idkptComputeSky (k_sky_atmosphere) at the reference's size and settings — HIP events around the launch on the context's stream, warm, repeated —
and idkptUpdateSky of a float and of an sRGB8 sky of the same size (wall time of the call, which does not wait for the GPU, and with the synchronisation that follows),
beside what the change replaces: the wall time of idkptUploadScene of soup-1M, the only way a new sky reached the library before.  The kernels' own lines: run this under
`rocprofv3 --kernel-trace --stats -- python tools/sky_timing.py --no-upload` and read k_sky_atmosphere / k_sky_expand.  Results: profiles/sky_atmosphere.md.

Usage: python tools/sky_timing.py [--size 128] [--reps 20] [--warmup 3] [--no-upload] [--upload-only] [--tris 1000000]
(IDKPT_LIB_PATH selects the library, e.g. a build of the parent commit for --upload-only.)"""
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
    ap.add_argument("--size", type=int, default=128); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tris", type=int, default=1000000); ap.add_argument("--no-upload", action="store_true"); ap.add_argument("--upload-only", action="store_true")
    a = ap.parse_args()
    import torch  # (one HIP runtime per process: torch's first)
    from idkengine_amd import gputypes as T, scenes as S, _lib
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    print(f"library: {_lib.LIB_PATH}  ABI {_lib.load().idkptGetAbiVersion()}", flush=True)
    if not a.no_upload:
        t0 = time.perf_counter(); big = S.soup_scene(a.tris, NativeBuilder(), seed=1); t1 = time.perf_counter()
        print(f"soup scene of {a.tris} triangles built on the host in {t1 - t0:.1f} s", flush=True)
        pt = PathTracer(64, 64); ts = []
        for i in range(1 + 5):                                          # (the first upload allocates)
            t0 = time.perf_counter(); pt.UploadScene(big); t1 = time.perf_counter()
            if i >= 1:
                ts.append((t1 - t0) * 1e3)
        print(f"idkptUploadScene soup-{a.tris}: {stats(ts)}  (5 uploads after 1)", flush=True)
        pt.Dispose(); del big
    if a.upload_only:
        return
    n = a.size
    pt = PathTracer(64, 64); pt.UploadScene(S.cornell_scene(NativeBuilder())); pt.SetCamera(S.cornell_camera(64, 64))
    stream = C.c_void_p(); pt._check(pt._L.idkptGetStream(pt._ctx, C.byref(stream)))
    ext = torch.cuda.ExternalStream(stream.value)
    atm = T.Atmosphere()
    ev, wall, wall_sync = [], [], []
    for i in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        atm.Azimuth = 0.01 * i                                          # a sun that moves
        t0 = time.perf_counter()
        e0.record(ext); pt.ComputeSky(n, atm); e1.record(ext)
        t1 = time.perf_counter(); pt.synchronize(); t2 = time.perf_counter()
        if i >= a.warmup:
            ev.append(e0.elapsed_time(e1)); wall.append((t1 - t0) * 1e3); wall_sync.append((t2 - t0) * 1e3)
    steps = 6 * n * n * atm.ISteps * atm.JSteps
    print(f"idkptComputeSky S = {n} ({6 * n * n} threads x {atm.ISteps * atm.JSteps} inner steps): k_sky_atmosphere by HIP events {stats(ev)}  ({np.median(ev) * 1e6 / steps:.3f} ns per inner step)", flush=True)
    print(f"    the call returns after {stats(wall)};  call + idkptSynchronize {stats(wall_sync)}  ({a.reps} launches after {a.warmup} warm)", flush=True)
    rng = np.random.default_rng(1)
    f32 = np.ones((6, n, n, 4), np.float32); f32[..., :3] = rng.uniform(0, 2, (6, n, n, 3))
    u8 = rng.integers(0, 256, (6, n, n, 4), dtype=np.uint8)
    for name, faces, fmt in (("RGBA32F", f32, T.IDKPT_TEXFMT_RGBA32F), ("SRGB8_A8", u8, T.IDKPT_TEXFMT_SRGB8_A8)):
        wall, wall_sync = [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter(); pt.UpdateSky(faces, fmt); t1 = time.perf_counter(); pt.synchronize(); t2 = time.perf_counter()
            if i >= a.warmup:
                wall.append((t1 - t0) * 1e3); wall_sync.append((t2 - t0) * 1e3)
        print(f"idkptUpdateSky {name:9s} S = {n} ({faces.nbytes / 2**20:.2f} MiB): the call returns after {stats(wall)};  call + idkptSynchronize {stats(wall_sync)}", flush=True)
    pt.ResetAccumulation(); pt.Compute(); assert np.isfinite(pt.Result).all()
    pt.Dispose()


if __name__ == "__main__":
    main()
