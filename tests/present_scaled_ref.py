"""Reference of the display chain at a presentation size other than the render size (idkptSetPresentationSize; csrc/kernels_present.hpp k_present_scaled, csrc/host_bloom.hpp),
written in numpy, independently of the kernels: Application.SetResolutions (Source/Application.cs:570-586) sizes PathTracer with the render resolution and Bloom and
TonemapAndGamma with the presentation resolution.

present_scaled(img, pw, ph, settings, add0, add1, dtype): what TonemapAndGammaCorrect/compute.glsl stores for every texel of a pw x ph ImgResult when Sampler0 holds the
(H, W, 4) image `img`: uv = (texel + 0.5) / (pw, ph); texture(Sampler0, uv) by the GL 4.6 8.14.2 linear filter with clamp to edge exactly as tests/bloom_ref.py writes it
(bloom_ref._tap: f = u * size - 0.5, floor, fractional weights, clamped indices, mix(x, y, a) = x * (1 - a) + y * a); then tests/present_ref.py present() on the sampled
image: the sum ((0 + s0) + s1) + s2 with add0 / add1 of the PRESENTATION size, AgX, sRGB and the dither of the presentation texel.  dtype as in present_ref: np.float32 is
the binary32 operation sequence, np.float64 the formula's value.
sampled_sum(...) is the value in front of the tone curve, ((0 + s0) + s1) + s2: everything the scaled path adds to idkptPresent, and free of exp / pow — the part a host
build of the shared filter (tests/c_driver/present_scaled_host.cpp) and the device reproduce bit for bit.
bloom_chain(img, pw, ph, settings, dtype): Bloom.Compute with a chain sized from the presentation size (Bloom.SetSize(presentRes)) whose first pass samples the render-size
image: bloom_ref.chain takes the sizes from its case and the source from the image it is given, so it is that function with the case (pw, ph, ...).

SIZES / CASE_IDS / SMALL / BLOOM_CHAINS name what tests/golden/present_scaled/*.npz holds (minted by tests/golden/make_present_scaled.py)."""
import os
import numpy as np
import bloom_ref as B
import present_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "present_scaled", "cases.npz")
BLOOM_FIXTURE = os.path.join(HERE, "golden", "present_scaled", "bloom.npz")

# ImgResult sizes for the 70 x 40 input of present_ref: non-integer magnifications (both width tails 93 = 1 mod 4, 71 = 3 mod 4), exactly x2, x10 (scale 0.1, the slider's
# end), one texel more than the source per axis, exactly half, and a minification by about 3 (supersampling)
SIZES = ((93, 53), (140, 80), (700, 400), (71, 41), (35, 20), (23, 13))
CASE_IDS = (0, 1, 9)                       # present_ref.CASES: the defaults, DoTonemapAndSrgbTransform = 0, the defaults with a bloom image as Sampler1
BIG = (700, 400)                           # held for CASE_IDS[0] only, and only its rows BIG_ROWS (the committed file stays small)
BIG_ROWS = np.arange(0, 400, 13)           # 13 is coprime to 8: every row phase of the dither
SMALL = ((3, 2), (9, 7))                   # a 3 x 2 input presented at 9 x 7: every output texel touches the clamped border
# powers of two the input is scaled by (with both signs) so that every value of the filtered sum — 3e-4 ... 1e4 in magnitude — lands in [2^-4, 1] once: in front of the clamp
SCALE_EXPONENTS = tuple(range(-14, 15, 4))
BLOOM_SETTINGS = (1.5, 3.8, 3)             # Threshold, MaxColor, MinusLods: the reference's defaults
# (W, H, pw, ph): source size, presentation size.  The engine's direction (render <= presentation) twice, supersampling (render > presentation: a tile of down pass 0
# would span more source texels than it stages, the direct-fetch route), and the smallest presentation size fed by a 3 x 2 source
BLOOM_CHAINS = ((70, 40, 93, 53), (70, 40, 140, 80), (70, 40, 23, 13), (3, 2, 2, 2))


def small_image():
    """(2, 3, 4) float32: six distinct colours, one exactly zero, one negative component, one above 1"""
    img = np.ones((2, 3, 4), np.float32)
    img[0, :, :3] = [[0.0, 0.0, 0.0], [0.25, 0.5, 0.75], [1.5, 0.125, -0.25]]
    img[1, :, :3] = [[0.9, 0.8, 0.1], [0.0625, 0.3, 0.6], [0.4, 2.0, 0.05]]
    return img


def bloom_image(pw, ph):
    """(ph, pw, 4) float32: present_ref.bloom_image()'s glow at the presentation size (Sampler1 has the presentation size)"""
    y = (np.arange(ph, dtype=np.float64) / max(ph - 1, 1))[:, None]; x = (np.arange(pw, dtype=np.float64) / max(pw - 1, 1))[None, :]
    g = 0.35 * np.exp(-((x - 0.5) ** 2 + (y - 0.5) ** 2) * 6.0)
    img = np.zeros((ph, pw, 4), np.float64); img[..., 0] = g; img[..., 1] = 0.8 * g; img[..., 2] = 0.5 * g + 0.01 * x; img[..., 3] = 1.0
    return img.astype(np.float32)


def sample(img, pw, ph, dtype=np.float32):
    """texture(Sampler0, (texel + 0.5) / (pw, ph)).rgb for every texel of a pw x ph image: (ph, pw, 3) of dtype"""
    src = np.asarray(img)[..., :3].astype(dtype)
    out = B._tap(src, B._coords(pw, dtype), B._coords(ph, dtype), 0, 0, dtype)
    assert out.dtype == np.dtype(dtype) and out.shape == (ph, pw, 3)
    return out


def sampled_sum(img, pw, ph, add0=None, add1=None, dtype=np.float32):
    """((0 + s0) + s1) + s2, (ph, pw, 3) of dtype: the value the tone curve receives"""
    f = dtype
    hdr = (np.zeros((ph, pw, 3), f) + sample(img, pw, ph, f)) + (add0[..., :3].astype(f) if add0 is not None else f(0.0))
    return hdr + (add1[..., :3].astype(f) if add1 is not None else f(0.0))


def present_scaled(img, pw, ph, settings, add0=None, add1=None, dtype=np.float32):
    """(ph, pw, 4) of dtype: vec4(ditherdColor, 1.0) for every texel of the presentation image"""
    s0 = np.ones((ph, pw, 4), dtype); s0[..., :3] = sample(img, pw, ph, dtype)
    return P.present(s0, settings, add0, add1, dtype)


def no_tonemap_display(hdr):
    """The RGBA32F display of DoTonemapAndSrgbTransform = 0 from the sampled sum `hdr` ((ph, pw, 3) float32): clamp to [0, 1], + dither — single binary32 operations"""
    assert hdr.dtype == np.float32
    ph, pw = hdr.shape[:2]
    d = P.dither_values(np.float32)
    out = np.ones((ph, pw, 4), np.float32)
    out[..., :3] = np.fmin(np.fmax(hdr, np.float32(0.0)), np.float32(1.0)) + d[(np.arange(pw) % 8)[None, :], (np.arange(ph) % 8)[:, None]][..., None]
    return out


def bloom_source(W, H):
    return B.input_image((W, H) + BLOOM_SETTINGS)


def bloom_chain(img, pw, ph, dtype=np.float32, settings=BLOOM_SETTINGS):
    return B.chain(img, (pw, ph) + tuple(settings), dtype)


def case_add(case_id, pw, ph):
    return bloom_image(pw, ph) if P.CASES[case_id][6] else None


def entries():
    """[(key, input image, (pw, ph), case id)] of the present fixture, in its order"""
    out = []
    for (pw, ph) in SIZES:
        for c in CASE_IDS:
            if (pw, ph) == BIG and c != CASE_IDS[0]:
                continue
            out.append((f"{pw}x{ph}_{c}", P.input_image(), (pw, ph), c))
    for c in CASE_IDS:
        out.append((f"small_{c}", small_image(), SMALL[1], c))
    return out


def fixture_entry(fx, key, pw, ph):
    """(rows, floats (len(rows), pw, 4), bytes (len(rows), pw, 4)) of an entry: llvmpipe's RGBA32F and R8G8B8A8Unorm ImgResult — all rows, or BIG_ROWS of the 700 x 400 entry"""
    f, b = fx["float_" + key], fx["bytes_" + key]
    rows = BIG_ROWS if (pw, ph) == BIG else np.arange(ph)
    assert f.shape == (len(rows), pw, 4) and f.dtype == np.float32 and b.shape == f.shape and b.dtype == np.uint8
    return rows, f, b


# ---- bounds: the rule of tests/test_present_ref.py and tests/test_bloom_ref.py, computed at run time -----------------------------------------------------------------------
def bound_of(fx, np32, np64, err=P.err):
    """(bound, e_gl, e_np) = (2 x max(e_gl, e_np), ...) against the binary64 evaluation: what a further binary32 execution — the device — may differ from it by"""
    e_gl, e_np = err(fx, np64), err(np32, np64)
    return 2.0 * max(e_gl, e_np), e_gl, e_np


def halves_within(bits, v64, b):
    """rtz(v64 - b) <= h <= rtz(v64 + b), per R, G, B, compared as values (the per-pass rule of stored halves)"""
    h = B.half_values(np.asarray(bits)[..., :3], np.float64)
    lo = B.half_values(B.rtz_half(v64 - b), np.float64); hi = B.half_values(B.rtz_half(v64 + b), np.float64)
    return (lo <= h) & (h <= hi)


def bloom_passes(fx, c):
    """[(name, chain, level, fixture bits, fixture floats, binary32 restatement, binary64 evaluation)] of chain c of bloom.npz in the order Bloom.Compute runs the passes;
    every pass is evaluated from the fixture's own input bits (tests/test_bloom_ref.py evaluate_passes, with the chain sized from the presentation size)."""
    W, H, pw, ph = BLOOM_CHAINS[c]
    thr, maxc, minus = BLOOM_SETTINGS
    levels, sz = B.sizes(pw, ph, minus)
    img = bloom_source(W, H)
    out = []
    for l in range(levels):
        ev = (lambda dt: B.down_pass0(img, sz[0], thr, maxc, dt)) if l == 0 else (lambda dt, l=l: B.down_pass(fx[f"down_bits_{c}_{l - 1}"], sz[l], dt, (thr, maxc) if l == 1 else None))
        out.append((f"down {l}", "down", l, fx[f"down_bits_{c}_{l}"], fx[f"down_f32_{c}_{l}"], ev(np.float32), ev(np.float64)))
    for l in range(levels - 2, -1, -1):
        a = fx[f"down_bits_{c}_{l + 1}"] if l == levels - 2 else fx[f"up_bits_{c}_{l + 1}"]
        ev = lambda dt, a=a, l=l: B.up_pass(a, fx[f"down_bits_{c}_{l + 1}"], sz[l], dt)
        out.append((f"up {l}", "up", l, fx[f"up_bits_{c}_{l}"], fx[f"up_f32_{c}_{l}"], ev(np.float32), ev(np.float64)))
    return out


# ---- the host build of the shared filter and texel functions (tests/c_driver/present_scaled_host.cpp) ------------------------------------------------------------------------
def build_host(directory):
    """present_scaled_host.cpp + csrc/bloom_texel.hpp under ASan and UBSan, as a stand-alone program; returns its path"""
    import subprocess
    exe = os.path.join(str(directory), "present_scaled_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           os.path.join(HERE, "c_driver", "present_scaled_host.cpp"), "-o", exe])
    return exe


def _run_host(exe, directory, mode, blob):
    import subprocess
    fin, fout = os.path.join(str(directory), "host.in"), os.path.join(str(directory), "host.out")
    with open(fin, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(fout, "rb") as f:
        return f.read()


def host_sum(exe, directory, img, pw, ph, adds=()):
    """((0 + s0) + s1) + s2 by the host program: (ph, pw, 3) float32"""
    H, W = img.shape[:2]
    blob = np.array([W, H, pw, ph, len(adds)], np.int32).tobytes() + np.ascontiguousarray(img, np.float32).tobytes() + b"".join(np.ascontiguousarray(a, np.float32).tobytes() for a in adds)
    raw = _run_host(exe, directory, "sum", blob)
    assert len(raw) == pw * ph * 12
    return np.frombuffer(raw, np.float32).reshape(ph, pw, 3).copy()


def host_bloom(exe, directory, img, pw, ph, settings=BLOOM_SETTINGS):
    """The chain by the host program: dict(levels, same, down = [bits], up = [bits], expand (ph, pw, 4) float32)"""
    H, W = img.shape[:2]
    blob = np.array([W, H, pw, ph, settings[2]], np.int32).tobytes() + np.array(settings[:2], np.float32).tobytes() + np.ascontiguousarray(img, np.float32).tobytes()
    raw = _run_host(exe, directory, "bloom", blob)
    levels, same = (int(v) for v in np.frombuffer(raw[:8], np.int32))
    want_levels, sz = B.sizes(pw, ph, settings[2])
    assert levels == want_levels
    off = 8; out = dict(levels=levels, same=same, down=[], up=[])
    for chain, n in (("down", levels), ("up", levels - 1)):
        for l in range(n):
            w, h = sz[l]
            out[chain].append(np.frombuffer(raw[off:off + w * h * 8], np.uint16).reshape(h, w, 4).copy()); off += w * h * 8
    out["expand"] = np.frombuffer(raw[off:], np.float32).reshape(ph, pw, 4).copy()
    return out
