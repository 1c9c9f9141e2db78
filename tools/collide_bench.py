"""Spheres per second of idkptCollideSpheres (k_collide_spheres) on soup-1M and the atrium, for 257 spheres with the lights' settings (TestSteps 1, RecursiveSteps 8,
epsilon 0.001, reflect) and for 1 M spheres, against the HOST build of the same header (tests/c_driver/collide_host.cpp, -O2, 16 threads) on the same spheres.  Device
times: a host clock around the device-pointer call plus idkptSynchronize (no copies: kernel + launch), and around the host-pointer call (with its copies); the launch
floor is the same call on one sphere far from the scene.  Outputs of device and host are compared byte for byte before anything is timed.  Results: profiles/collide.md.

Usage: python tools/collide_bench.py [--tris 1000000] [--big 1000000] [--reps 9] [--threads 16] [--scenes soup,atrium]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import collide_ref as R  # noqa: E402  (the host program's input format)
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd.bvh import NativeBuilder  # noqa: E402
from idkengine_amd.pathtracer import PathTracer  # noqa: E402

KW = dict(test_steps=1, recursive_steps=8, epsilon=0.001, response=2, use_tlas=False)


def spheres_for(sc, n, seed):
    """light-like spheres inside the scene's bounds: radius 0.1 .. 0.5, one frame's movement (up to 0.3) in a random direction"""
    lo, hi = sc.vertex_positions.min(0), sc.vertex_positions.max(0)
    rng = np.random.default_rng(seed)
    prev = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    dest = (prev + d * rng.uniform(0, 0.3, (n, 1))).astype(np.float32)
    return R.make_spheres(prev, rng.uniform(0.1, 0.5, n).astype(np.float32), dest)


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000); ap.add_argument("--big", type=int, default=1_000_000); ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16); ap.add_argument("--scenes", default="soup,atrium")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("collide_bench.py needs a GPU")
    tmp = tempfile.mkdtemp(prefix="collide_bench")
    exe = os.path.join(tmp, "collide_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DCOLLIDE_THREADS", "-pthread", os.path.join(ROOT, "tests", "c_driver", "collide_host.cpp"), "-o", exe])
    builder = NativeBuilder()
    dev = torch.device("cuda", 0)
    for name in a.scenes.split(","):
        sc = S.soup_scene(a.tris, builder, seed=1) if name == "soup" else S.atrium_scene(a.tris, builder)
        pt = PathTracer(8, 8); pt.UploadScene(sc)
        far = R.make_spheres([(1e6, 1e6, 1e6)], 0.25, [(1e6, 1e6 + 0.1, 1e6)])
        d_far = torch.from_numpy(np.frombuffer(far.tobytes(), np.uint8).copy()).to(dev)
        m, lo, hi = timed(lambda: pt.CollideSpheres(d_far, **KW), a.reps * 3)
        print(f"{name} ({len(sc.blas_triangles)} triangles): launch floor (1 sphere out of reach, device pointers, call + synchronise): median {m * 1e6:.1f} us  min {lo * 1e6:.1f}  max {hi * 1e6:.1f}")
        for n in (257, a.big):
            sp = spheres_for(sc, n, 5)
            d_in = torch.from_numpy(np.frombuffer(sp.tobytes(), np.uint8).copy()).to(dev)
            src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(src, "wb") as f:
                f.write(R.host_input(sc, sp, KW["test_steps"], KW["recursive_steps"], KW["epsilon"], KW["response"], KW["use_tlas"]))
            cpu = float(subprocess.check_output([exe, src, dst, str(a.threads), str(max(3, a.reps // 3))]).decode())
            got = pt.CollideSpheres(sp, **KW)
            same = got.tobytes() == open(dst, "rb").read()
            hits = int((got["HitCount"] > 0).sum())
            dm, dlo, dhi = timed(lambda: pt.CollideSpheres(d_in, **KW), a.reps)
            hm, hlo, hhi = timed(lambda: pt.CollideSpheres(sp, **KW), a.reps)
            print(f"{name} {n} spheres ({hits} collide; device == host build: {same}):")
            print(f"    device pointers  median {dm * 1e3:9.4f} ms  min {dlo * 1e3:9.4f}  max {dhi * 1e3:9.4f}   {n / dm / 1e6:9.3f} M spheres/s")
            print(f"    host pointers    median {hm * 1e3:9.4f} ms  min {hlo * 1e3:9.4f}  max {hhi * 1e3:9.4f}   {n / hm / 1e6:9.3f} M spheres/s")
            print(f"    CPU, {a.threads} threads   best   {cpu * 1e3:9.4f} ms                                {n / cpu / 1e6:9.3f} M spheres/s")
            if not same:
                sys.exit("device and host build disagree")
        pt.Dispose()


if __name__ == "__main__":
    main()
