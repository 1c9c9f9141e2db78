"""Tunes LumaSigma and VarianceEpsilon of idkptDenoiseVariance on the CPU and measures its quality beside idkptDenoise's: tests/denoise_variance_ref.py and
tests/denoise_ref.py (the binary32 restatements of the two filters) applied to few-sample renders of the 64 x 64 Cornell box, scored by the RMSE against a converged render
of the same view.  The sibling of tools/denoise_tune.py; that tool's fixture has no moments, so this one has its own.

  python tools/denoise_variance_tune.py --mint     renders the fixture tests/golden/denoise/cornell64_moments.npz WITH THE LIBRARY (needs a GPU: the moments are what
                                                   FinalDraw keeps under idkptSetNoiseEstimate): Result / Albedo / Normal / moments at 4 and at 16 samples, Result at 4096
  python tools/denoise_variance_tune.py            the search over LumaSigma x VarianceEpsilon (Iterations 5, DemodulateAlbedo 1, the guide sigmas of idkptDenoise) at both
                                                   sample counts, and idkptDenoise's defaults on the same frames; prints what profiles/denoise_variance.md quotes
"""
import argparse
import itertools
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_ref as D  # noqa: E402
import denoise_variance_ref as R  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "denoise", "cornell64_moments.npz")
W = H = 64
NOISY_SAMPLES, CONVERGED_SAMPLES, RAY_DEPTH = (4, 16), 4096, 4


def mint(path):
    from idkengine_amd import scenes as S
    from idkengine_amd.bvh import NativeBuilder
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(W, H)
    pt.UploadScene(S.cornell_scene(NativeBuilder(), variant="mixed")); pt.SetCamera(S.cornell_camera(W, H)); pt.RayDepth = RAY_DEPTH; pt.OutputAOVs = 1
    pt.SetNoiseEstimate(True)
    out = {}
    for i in range(CONVERGED_SAMPLES):
        pt.Compute()
        if i + 1 in NOISY_SAMPLES:
            assert pt.AccumulatedSamples == i + 1
            for name, im in zip(("result", "albedo", "normal"), (pt.FrameResult(0, k) for k in range(3))):
                out[f"{name}{i + 1}"] = im
            out[f"moments{i + 1}"] = pt.DownloadMoments()
    out["converged"] = pt.FrameResult(0, 0)
    pt.Dispose()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, samples=np.array(list(NOISY_SAMPLES) + [CONVERGED_SAMPLES, RAY_DEPTH], np.int32), **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mint", action="store_true")
    ap.add_argument("--fixture", default=FIXTURE)
    args = ap.parse_args()
    if args.mint:
        mint(args.fixture)
        return
    fx = np.load(args.fixture)
    conv = fx["converged"]
    frames = {n: (fx[f"result{n}"], fx[f"albedo{n}"], fx[f"normal{n}"], fx[f"moments{n}"]) for n in NOISY_SAMPLES}
    before = {n: rmse(frames[n][0], conv) for n in NOISY_SAMPLES}
    for n in NOISY_SAMPLES:
        plain = rmse(D.denoise(*frames[n][:3], **D.DEFAULTS), conv)
        print(f"{n} samples against {CONVERGED_SAMPLES}: unfiltered RMSE {before[n]:.6f}; idkptDenoise defaults {plain:.6f} (x {plain / before[n]:.3f})")
    rows = []
    for ls, eps in itertools.product([0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0], [1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 10.0, 100.0]):
        r = [rmse(R.denoise_variance(*frames[n], n, 5, ls, eps, 0.2, 0.5, 1), conv) / before[n] for n in NOISY_SAMPLES]
        rows.append((float(np.sqrt(r[0] * r[1])), r[0], r[1], ls, eps))
    rows.sort()
    print("best 12 of", len(rows), f"(geometric mean of the two ratios, ratio at {NOISY_SAMPLES[0]}, ratio at {NOISY_SAMPLES[1]} samples, LumaSigma, VarianceEpsilon):")
    for row in rows[:12]:
        print("  %.4f  %.4f  %.4f  %-5s %s" % row)
    print("worst: %.4f  %.4f  %.4f  %-5s %s" % rows[-1])
    d = R.DEFAULTS
    for n in NOISY_SAMPLES:
        o = rmse(R.denoise_variance(*frames[n], n, **d), conv)
        print(f"the defaults {d} at {n} samples: RMSE {o:.6f}, ratio {o / before[n]:.3f}")
        print("  Iterations 1..6:", " ".join(f"{rmse(R.denoise_variance(*frames[n], n, **dict(d, Iterations=it)), conv) / before[n]:.3f}" for it in range(1, 7)))


if __name__ == "__main__":
    main()
