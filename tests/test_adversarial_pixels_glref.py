"""The reference's own shaders on the adversarial pixels: tests/golden/adversarial_pixels/{present,bloom}.npz hold what Shaders/TonemapAndGammaCorrect/compute.glsl and
Shaders/Bloom/compute.glsl give on Mesa llvmpipe for every case of tests/adversarial_pixels.py (minted by tests/golden/make_adversarial_pixels.py; outputs only).

  * Finite classes (flt_max, subnormal32, neg_zero, negative, half_edges) are held to the bounds the project measured against llvmpipe per pass, in the form of
    tests/test_present_ref.py and tests/test_bloom_ref.py: b = 2 x the larger error of the two binary32 executions against the binary64 value.  Texels that fetch a planted
    FLT_MAX are left to the table below: binary32 overflows there (FLT_MAX * 2^Exposure; sums of FLT_MAX taps) where binary64 does not, so binary64 is no yardstick and what
    follows the overflow is as undefined in GLSL as for a planted Inf.
  * The half store: llvmpipe's RGBA16F bits are the header's rule applied to llvmpipe's own floats on EVERY texel of every class — round toward zero, 65504 beyond, subnormals,
    +-Inf kept, NaN -> sign | 0x7E00 — with the boundary values of half_edges on the exact bit patterns the generator lists.
  * Non-finite classes through arithmetic: tests/golden/adversarial_pixels/table.json records, per family and class, what llvmpipe gives where the restatement gives a
    non-finite value (bloom), and on how many texels its display is another colour than the restatement's (display pass).  GLSL leaves this undefined: information, not a
    pass condition; the test pins the committed table to the committed fixture.  (python tests/test_adversarial_pixels_glref.py --write  regenerates the table.)
  * live: the fixture is reproducible where the reference and llvmpipe exist."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adversarial_pixels as A  # noqa: E402
import bloom_ref as B  # noqa: E402
import present_ref as P  # noqa: E402
import present_scaled_ref as S  # noqa: E402
from test_bloom_ref import pass_bound, halves_within, live  # noqa: E402
from test_present_ref import present_bound  # noqa: E402

f32 = np.float32
DIR = os.path.join(HERE, "golden", "adversarial_pixels")
TABLE = os.path.join(DIR, "table.json")
OTHER_COLOUR = 2.0 ** -8                                   # one display step: far beyond any rounding difference (1e-5), far below a saturated-against-black difference (1)


def size_id(size):
    return f"{size[0]}x{size[1]}" + (f"_{size[2]}x{size[3]}" if len(size) == 4 else "")


DISPLAYS = [("present", s) for s in A.PRESENT_SIZES] + [("scaled", s) for s in A.SCALED_SIZES]
BLOOMS = [("bloom", s) for s in A.BLOOM_SIZES] + [("scaled", s) for s in A.SCALED_SIZES]


@pytest.fixture(scope="module")
def fx_present():
    return np.load(os.path.join(DIR, "present.npz"))


@pytest.fixture(scope="module")
def fx_bloom():
    return np.load(os.path.join(DIR, "bloom.npz"))


def restated_display(c, tm, adds, dt):
    a0, a1 = (c.add0, c.add1) if adds else (None, None)
    with np.errstate(all="ignore"):
        return P.present(c.img, tm, a0, a1, dt) if c.family == "present" else S.present_scaled(c.img, c.size[2], c.size[3], tm, a0, a1, dt)


def touched(c):
    """(ph, pw) bool: the display texels that fetch a texel planted into the image or an added image"""
    pw, ph = (c.size[2], c.size[3]) if c.family == "scaled" else c.size
    m = np.zeros((ph, pw), bool)
    for t, r, k, _ in c.planted:
        if t != "img" or c.family == "present":
            m[r, k] = True
        else:
            m |= A.scaled_footprint(c.size, r, k)
    # llvmpipe's texture() filters with weights of limited precision (profiles/present.md): at a texel centre a neighbour still enters with a weight of about 2^-8 or less,
    # which FLT_MAX survives.  So on llvmpipe a planted texel also reaches the texels next to the ones that fetch it: one ring more is left to the table.
    d = m.copy()
    d[1:] |= m[:-1]; d[:-1] |= m[1:]
    e = d.copy()
    e[:, 1:] |= d[:, :-1]; e[:, :-1] |= d[:, 1:]
    return e


def bloom_passes(fb, fam, size, i, c):
    """[(name, chain, level, fixture bits, fixture floats, binary32 restatement, binary64 evaluation)] of class i, every pass from the fixture's own input bits"""
    pre = f"b_{fam}_{size_id(size)}_"
    W, H, thr, maxc, minus = A.bloom_case(c)
    levels, sz = B.sizes(W, H, minus)
    g = lambda k: fb[pre + k][i]
    out = []
    with np.errstate(all="ignore"):
        for l in range(levels):
            ev = (lambda dt: B.down_pass0(c.img, sz[0], thr, maxc, dt)) if l == 0 else (lambda dt, l=l: B.down_pass(g(f"down_{l - 1}_bits"), sz[l], dt, (thr, maxc) if l == 1 else None))
            out.append((f"down {l}", "down", l, g(f"down_{l}_bits"), g(f"down_{l}_f32"), ev(f32), ev(np.float64)))
        for l in range(levels - 2, -1, -1):
            a = g(f"down_{l + 1}_bits") if l == levels - 2 else g(f"up_{l + 1}_bits")
            ev = lambda dt, a=a, l=l: B.up_pass(a, g(f"down_{l + 1}_bits"), sz[l], dt)
            out.append((f"up {l}", "up", l, g(f"up_{l}_bits"), g(f"up_{l}_f32"), ev(f32), ev(np.float64)))
    return out


def test_fixture_covers_every_case(fx_present, fx_bloom):
    n = len(A.CLASSES)
    for fam, size in DISPLAYS:
        pw, ph = (size[2], size[3]) if fam == "scaled" else size
        f, u = fx_present[f"p_{fam}_{size_id(size)}_f32"], fx_present[f"p_{fam}_{size_id(size)}_u8"]
        assert f.shape == (n, len(A.TONEMAPS), 2, ph, pw, 4) and f.dtype == f32 and u.shape == f.shape and u.dtype == np.uint8
        assert (f[..., 3] == 1.0).all() and (u[..., 3] == 255).all()
    for fam, size in BLOOMS:
        c = A.case(fam, size, "nan")
        levels, sz = B.sizes(*A.bloom_case(c)[:2], A.BLOOM_MINUS_LODS)
        assert levels >= 3 or fam == "scaled"
        for l in range(levels):
            assert fx_bloom[f"b_{fam}_{size_id(size)}_down_{l}_bits"].shape == (n, sz[l][1], sz[l][0], 4)
        assert f"b_{fam}_{size_id(size)}_up_{levels - 2}_bits" in fx_bloom.files and f"b_{fam}_{size_id(size)}_up_{levels - 1}_bits" not in fx_bloom.files


def test_finite_classes_of_the_display_pass_sit_inside_the_measured_bound(fx_present):
    """The form of tests/test_present_ref.py: both binary32 executions within b = 2 x max(e_gl, e_np) of the binary64 value, and b below half an 8-bit step.  Over the whole
    image for every finite class but flt_max, whose planted texels overflow in binary32 (see the module docstring); there over the texels no planted texel reaches."""
    for fam, size in DISPLAYS:
        f = fx_present[f"p_{fam}_{size_id(size)}_f32"]
        for cls in A.FINITE_CLASSES:
            i = A.CLASSES.index(cls); c = A.case(fam, size, cls)
            for t, tm in enumerate(A.TONEMAPS):
                for adds in (0, 1):
                    fx = f[i, t, adds]
                    r32, r64 = restated_display(c, tm, adds, f32), restated_display(c, tm, adds, np.float64)
                    keep = ~touched(c) if cls == "flt_max" else np.ones(fx.shape[:2], bool)
                    b, e_gl, e_np = present_bound(fx[keep], r32[keep], r64[keep])
                    print(f"{fam} {size_id(size)} {cls} tone {t} adds {adds}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {b:.3e}")
                    assert np.isfinite(fx).all() and e_gl <= b and e_np <= b and b < 1.0 / 510.0, (fam, size, cls, t, adds, b)


def test_finite_classes_of_bloom_sit_inside_the_measured_bound(fx_bloom):
    """The form of tests/test_bloom_ref.py, per pass from the fixture's own input bits: b <= 2^-12 of the pass's largest value, and both executions' halves inside
    rtz(T -+ b).  flt_max is left to the table (its taps overflow in binary32 and not in binary64)."""
    for fam, size in BLOOMS:
        for cls in A.FINITE_CLASSES:
            if cls == "flt_max":
                continue
            i = A.CLASSES.index(cls); c = A.case(fam, size, cls)
            for name, chain, l, bits, g32, np32, np64 in bloom_passes(fx_bloom, fam, size, i, c):
                m = np.isfinite(np32).all(axis=-1)         # (class negative holds -1e30 and -3e38: a few sums overflow in binary32; those texels are the table's)
                assert m.sum() >= 0.8 * m.size and np.isfinite(g32[m]).all() and np.isfinite(np64[m]).all(), (fam, size, cls, name)
                b, e_gl, e_np = pass_bound(g32[m], np32[m], np64[m])
                scale = float(np.abs(np64[m]).max())
                print(f"{fam} {size_id(size)} {cls} {name}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {b:.3e}  (largest value {scale:.4g})")
                assert b <= 2.0 ** -12 * scale, (fam, size, cls, name, b, scale)
                assert halves_within(bits[m], np64[m], b).all() and halves_within(B.store(np32)[m], np64[m], b).all(), (fam, size, cls, name)


def test_llvmpipe_stores_halves_by_the_headers_rule_inf_and_nan_included(fx_bloom):
    """Every texel of every level of every class: bits == rule(llvmpipe's own floats), Inf and NaN by class and sign; half_edges on the listed bit patterns."""
    seen = dict(nan=0, pinf=0, ninf=0)
    for fam, size in BLOOMS:
        for k in fx_bloom.files:
            if not (k.startswith(f"b_{fam}_{size_id(size)}_") and k.endswith("_f32")):
                continue
            g32, bits = fx_bloom[k][..., :3], fx_bloom[k.replace("_f32", "_bits")]
            assert (bits[..., 3] == 0x3C00).all()
            want = B.rtz_half(g32)
            ok = A.same_half(bits[..., :3], want)
            assert ok.all(), (k, np.argwhere(~ok)[:3].tolist())
            assert ((bits[..., :3] & 0x8000 != 0) == np.signbit(g32))[np.isnan(g32)].all()          # the stored NaN keeps llvmpipe's own sign
            seen["nan"] += int(np.isnan(g32).sum()); seen["pinf"] += int(np.isposinf(g32).sum()); seen["ninf"] += int(np.isneginf(g32).sum())
    # the statement is about something: llvmpipe stored NaN and -Inf.  No +Inf ever reaches a store in these chains (Prefilter's min(MaxColor, c) takes it away in the
    # first pass), so the fixture cannot speak about +Inf, and the header does not.
    assert seen["nan"] > 0 and seen["ninf"] > 0 and seen["pinf"] == 0, seen
    for size in A.HALF_EDGE_EXACT_SIZES:
        d0 = fx_bloom[f"b_bloom_{size_id(size)}_down_0_bits"][A.CLASSES.index("half_edges")]
        for (r, k), (v, h) in zip(A.HALF_EDGE_TEXELS, A.HALF_EDGES):
            assert d0[r, k].tolist() == [0x7BFF, h, h | 0x8000, 0x3C00], (r, k, float(v), d0[r, k].tolist())


def kind(x):
    return np.where(np.isnan(x), 0, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 3)))


KINDS = ("NaN", "+Inf", "-Inf", "finite")


def compute_table(fp, fb):
    """{"bloom": {family: {class: {"restatement -> llvmpipe": values}}}, "display": {family: {class: [texels of another colour, texels]}}}, summed over sizes, passes, settings"""
    tab = {"bloom": {}, "display": {}}
    for fam, size in BLOOMS:
        for i, cls in enumerate(A.CLASSES):
            c = A.case(fam, size, cls)
            row = tab["bloom"].setdefault(fam, {}).setdefault(cls, {})
            for name, chain, l, bits, g32, np32, np64 in bloom_passes(fb, fam, size, i, c):
                kn, kg = kind(np32), kind(g32[..., :3])
                for a in range(3):
                    for b in range(4):
                        n = int(((kn == a) & (kg == b)).sum())
                        if n:
                            key = f"{KINDS[a]} -> {KINDS[b]}"
                            row[key] = row.get(key, 0) + n
    for fam, size in DISPLAYS:
        f = fp[f"p_{fam}_{size_id(size)}_f32"]
        for i, cls in enumerate(A.CLASSES):
            c = A.case(fam, size, cls)
            row = tab["display"].setdefault(fam, {}).setdefault(cls, [0, 0, 0])
            for t, tm in enumerate(A.TONEMAPS):
                for adds in (0, 1):
                    d = np.abs(f[i, t, adds].astype(np.float64) - restated_display(c, tm, adds, f32))[..., :3].max(axis=-1)
                    row[0] += int((d > OTHER_COLOUR).sum()); row[1] += int(d.size); row[2] += int((~np.isfinite(f[i, t, adds])).sum())
    return tab


def test_committed_table_matches_the_committed_fixture(fx_present, fx_bloom):
    with open(TABLE) as fh:
        assert json.load(fh) == json.loads(json.dumps(compute_table(fx_present, fx_bloom)))


@live
def test_live_fixture_is_reproducible():
    """Runs the reference's shaders on llvmpipe again and demands the committed fixtures bit for bit (separate process: Mesa brings its own LLVM)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_adversarial_pixels.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__" and "--write" in sys.argv:
    with open(TABLE, "w") as fh:
        json.dump(compute_table(np.load(os.path.join(DIR, "present.npz")), np.load(os.path.join(DIR, "bloom.npz"))), fh, indent=1, sort_keys=True)
    print("wrote", TABLE)
