"""Tunes the sigma defaults of idkptDenoise on the CPU: tests/denoise_ref.py (the binary32 restatement of the filter) applied to a few-sample CPU-oracle render of the
64 x 64 Cornell box, scored by the RMSE against the oracle's converged render of the same view.  No GPU is involved.

  python tools/denoise_tune.py --mint      renders the fixture tests/golden/denoise/cornell64.npz (noisy Result / Albedo / Normal at 4 samples, Result at 1024)
  python tools/denoise_tune.py             the search over ColorSigma x AlbedoSigma x NormalSigma (Iterations 5, DemodulateAlbedo 1); writes what profiles/denoise.md quotes
"""
import argparse
import itertools
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_ref as R  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "denoise", "cornell64.npz")
W = H = 64
NOISY_SAMPLES, CONVERGED_SAMPLES, RAY_DEPTH = 4, 1024, 4


def mint():
    from idkengine_amd import scenes as S
    from idkengine_amd.bvh import NativeBuilder
    from oracle import oracle as O
    O.build()
    sc = S.cornell_scene(NativeBuilder(), variant="mixed")
    cam = S.cornell_camera(W, H)
    ref = O.OraclePathTracer(sc, W, H)
    ref.set_camera(cam); ref.settings.RayDepth = RAY_DEPTH; ref.settings.OutputAOVs = 1
    out = {}
    for i in range(CONVERGED_SAMPLES):
        ref.render()
        if i + 1 == NOISY_SAMPLES:
            out["result"], out["albedo"], out["normal"] = ref.image(0), ref.image(1), ref.image(2)
    out["converged"] = ref.image(0)
    ref.close()
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    np.savez_compressed(FIXTURE, samples=np.array([NOISY_SAMPLES, CONVERGED_SAMPLES, RAY_DEPTH], np.int32), **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mint", action="store_true")
    args = ap.parse_args()
    if args.mint:
        mint()
        return
    fx = np.load(FIXTURE)
    before = rmse(fx["result"], fx["converged"])
    print(f"RMSE of the {int(fx['samples'][0])}-sample render against the {int(fx['samples'][1])}-sample one: {before:.6f}")
    rows = []
    for cs, as_, ns in itertools.product([0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0], [0.05, 0.1, 0.2, 0.4, 0.8], [0.125, 0.25, 0.5, 1.0]):
        out = R.denoise(fx["result"], fx["albedo"], fx["normal"], 5, cs, as_, ns, 1)
        rows.append((rmse(out, fx["converged"]), cs, as_, ns))
    rows.sort()
    print("best 12 of", len(rows), "(RMSE, ratio to the unfiltered, ColorSigma, AlbedoSigma, NormalSigma):")
    for r, cs, as_, ns in rows[:12]:
        print(f"  {r:.6f}  {r / before:.3f}  {cs:<5} {as_:<6} {ns}")
    print("worst:", " ".join(f"{v}" for v in rows[-1]))
    d = R.DEFAULTS
    out = R.denoise(fx["result"], fx["albedo"], fx["normal"], **d)
    print(f"the defaults {d}: RMSE {rmse(out, fx['converged']):.6f}, ratio {rmse(out, fx['converged']) / before:.3f}")
    for it in (1, 2, 3, 4, 5, 6):
        o = R.denoise(fx["result"], fx["albedo"], fx["normal"], **dict(d, Iterations=it))
        print(f"  Iterations {it}: ratio {rmse(o, fx['converged']) / before:.3f}")
    o = R.denoise(fx["result"], fx["albedo"], fx["normal"], **dict(d, DemodulateAlbedo=0))
    print(f"  DemodulateAlbedo 0: ratio {rmse(o, fx['converged']) / before:.3f}")


if __name__ == "__main__":
    main()
