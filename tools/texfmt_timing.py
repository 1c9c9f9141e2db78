"""idkptUpdateTexture of one size x size image in a storage format the library decodes on the device (BC7, R8) against the RGBA8 upload a host had to make before:
wall time around the (synchronising) call, warm, repeated; median and spread.  The decode kernels' own time: run this under `rocprofv3 --kernel-trace --stats -- python
tools/texfmt_timing.py` and read k_tex_decode_bc7 / k_tex_expand_linear.  Results: profiles/texfmt_decode.md.

Usage: python tools/texfmt_timing.py [--size 4096] [--reps 15] [--warmup 3]"""
import argparse
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096); ap.add_argument("--reps", type=int, default=15); ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    from idkengine_amd import gputypes as T, scenes as S
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    import texfmt_ref as R
    n = a.size; rng = np.random.default_rng(1)
    blocks, _ = R.bc7_fixture()
    bc7 = blocks[rng.integers(0, len(blocks), (n // 4) * (n // 4))]
    images = [("BC7_SRGBA", T.TextureImage.from_storage(T.IDKPT_TEXFMT_BC7_SRGBA, n, n, bc7)),
              ("R8", T.TextureImage.from_storage(T.IDKPT_TEXFMT_R8, n, n, rng.integers(0, 256, n * n, dtype=np.uint8))),
              ("RGBA8", T.TextureImage(rng.integers(0, 256, (n, n, 4), dtype=np.uint8)))]
    sc = S.cornell_scene(NativeBuilder(), variant="mixed"); sc.textures = [np.zeros((1, 1, 4), np.float32)]
    pt = PathTracer(64, 64); pt.UploadScene(sc)
    for name, img in images:
        ts = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter(); pt.UpdateTexture(0, img); t1 = time.perf_counter()
            if i >= a.warmup:
                ts.append((t1 - t0) * 1e3)
        ts = np.array(ts)
        print(f"{name:10s} {n}x{n}  in {img.data.nbytes / 2**20:6.1f} MiB  median {np.median(ts):8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}  ({a.reps} reps after {a.warmup} warm)", flush=True)
    pt.Dispose()


if __name__ == "__main__":
    main()
