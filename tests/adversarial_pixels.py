"""Adversarial pixels for the display chain (idkptBloom, idkptPresent, the scaled display pass of idkptSetPresentationSize): the texel values a path tracer can leave in
`Result` and that nothing downstream was tested on — NaN, +-Inf, FLT_MAX, sums that overflow, binary32 subnormals, -0, negatives, and the values on the half-precision
boundaries.  numpy only, deterministic; the shape of the other adversarial_*.py modules: named classes, each planted into an otherwise ordinary finite image taken from
present_ref.input_image() / bloom_ref.input_image(), and a table {class: [(row, col)]} of where.

The rule the kernels and the restatements (tests/present_ref.py, tests/present_scaled_ref.py, tests/bloom_ref.py) are held to is written in include/idkpt.h ("Non-finite and
extreme texels") and profiles/display_nonfinite.md.  Addresses in these kernels come from texel coordinates and sizes only: a texel's VALUE never feeds an index.

  case(family, size, cls) -> Case     family "present": size (W, H);  "bloom": size (W, H);  "scaled": size (W, H, pw, ph) — a W x H image presented at pw x ph
  table(family, size)     -> {class: [(row, col)]}
Case.img is the image (H, W, 4) float32; Case.add0 / add1 the Sampler1 / Sampler2 images of the display pass (presentation size), ordinary finite glows except where class
overflowing_sum plants into them; Case.planted lists (target, row, col, (r, g, b) as binary32 bit patterns) for every planted texel, target in "img" / "add0" / "add1";
Case.positions the (row, col) of the texels planted into img; Case.bloom the (Threshold, MaxColor, MinusLods) the class wants for idkptBloom.

Class zero_weight is planted only where the pass that reads the image HAS a tap weight of exactly 0 (zero_weight_taps): bloom at 33 x 19 and the scaled pass at 9 x 5 ->
15 x 7.  At every other size — the three scaled sizes 12 x 8 -> 18 x 10 / 7 x 5 / 24 x 16 among them, whose weights are never 0 — its image is the base image and its list
in table() is empty.

Equality (same_value of tests/adversarial_surfaces.py for binary32; same_half here for stored halves): equal bits; or both NaN — the sign of a NaN that ARITHMETIC makes is
the platform's (inf * 0 is 0xFFC00000 on x86 and 0x7FC00000 on the device), so binary32 NaNs compare as a class and a stored half NaN, which the header's rule makes
sign | 0x7E00, compares on its low 15 bits —; or both the same signed infinity.  No texel is left out of a comparison."""
import collections
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bloom_ref as B  # noqa: E402
import present_ref as P  # noqa: E402
from adversarial_surfaces import same_value  # noqa: E402,F401  (re-exported: the binary32 equality of this suite)

f32 = np.float32
CLASSES = ("nan", "pos_inf", "neg_inf", "inf_pair", "flt_max", "overflowing_sum", "subnormal32", "neg_zero", "negative", "half_edges", "edge_texels", "zero_weight", "isolated")
FINITE_CLASSES = ("flt_max", "subnormal32", "neg_zero", "negative", "half_edges")           # every planted value finite (overflowing_sum: finite inputs, infinite sums)

# sizes: the smallest at which each kernel's shapes still differ
PRESENT_SIZES = ((9, 5), (16, 8))                          # k_present: the W mod 4 row tail; the full 16-byte store
BLOOM_SIZES = ((24, 16), (33, 19))                         # an even chain (12 x 8, 6 x 4, 3 x 2); odd sizes at every level (16 x 9, 8 x 4, 4 x 2, 2 x 1)
BLOOM_MINUS_LODS = 1                                       # three and four down levels
# magnify; supersample; exactly x2 (weights 0.25 / 0.75 inside, clamped pairs at the border); odd to odd, whose centre column and row (u = 0.5, an odd source size) have a
# weight of exactly 0; and a supersampling wide enough that a tile of bloom's first pass spans more source texels than k_bloom_down0 stages (44 > 40): k_bloom_down0_direct
SCALED_SIZES = ((12, 8, 18, 10), (12, 8, 7, 5), (12, 8, 24, 16), (9, 5, 15, 7), (56, 8, 7, 5))
DIRECT_ROUTE_SIZES = ((56, 8, 7, 5),)
# (Exposure, Saturation, Linear, Peak, Compression, DoTonemapAndSrgbTransform): the defaults, the path without the tone curve, and Linear 0 (DualSection's S = 0)
TONEMAPS = (P.DEFAULTS, P.DEFAULTS[:5] + (0,), (0.45, 1.06, 0.0, 1.0, 0.1, 1))
BLOOM_DEFAULTS = (1.5, 3.8)                                # Threshold, MaxColor
FLT_MAX_BITS = 0x7F7FFFFF
# Prefilter with Threshold 0 and MaxColor FLT_MAX: a texel whose largest channel b is >= 0.2 and < FLT_MAX has rq = 0.4^2 * 1.25 = 0.2 <= b, s = b / b = 1, c * 1 = c
HALF_EDGE_BLOOM = (0.0, float(np.array(FLT_MAX_BITS, np.uint32).view(f32)))

QNAN, SNAN, NEG_NAN, PAYLOAD_NAN = 0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FC12345     # quiet, signalling pattern, negative sign, quiet with a payload
POS_INF, NEG_INF = 0x7F800000, 0xFF800000
NEG_ZERO = 0x80000000

# Anything that exposed a product bug: {name: (family, size, class, (row, col))}.  Kept by name, as REGRESSION_RAYS is.  None so far: what the first runs found were the
# restatements' NaN conventions, not the kernels' (profiles/display_nonfinite.md).
REGRESSION_PIXELS = {}

Case = collections.namedtuple("Case", "family size cls img add0 add1 planted positions bloom")


def fb(x):
    """the binary32 bit pattern of a float"""
    return int(np.array(x, f32).view(np.uint32))


def bf(u):
    """the binary32 value of a bit pattern"""
    return np.array(u, np.uint32).view(f32)[()]


def below(x):
    """the last binary32 value below x > 0"""
    return np.nextafter(f32(x), f32(0.0))


def same_half(a, b):
    """elementwise on RGBA16F bits: equal, or both the rule's NaN (sign | 0x7E00) — the sign is the binary32 NaN's, which arithmetic leaves to the platform"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint16 and b.dtype == np.uint16 and a.shape == b.shape
    return (a == b) | (((a & 0x7FFF) == 0x7E00) & ((b & 0x7FFF) == 0x7E00))


# ---- the half-precision boundaries: (binary32 value, the half the rule stores for +value); -value stores the same bits | 0x8000
HALF_EDGES = (
    (f32(65504.0), 0x7BFF), (below(65504.0), 0x7BFE), (below(65520.0), 0x7BFF), (f32(65520.0), 0x7BFF), (f32(65536.0), 0x7BFF), (below(65536.0), 0x7BFF),
    (f32(2.0 ** -24), 0x0001), (below(2.0 ** -24), 0x0000), (f32(2.0 ** -25), 0x0000), (below(2.0 ** -25), 0x0000), (f32(2.0 ** -14), 0x0400), (below(2.0 ** -14), 0x03FF),
)
HALF_EDGE_DRIVER = f32(131072.0)                           # R of every half_edges patch of the bloom family: the largest channel, so that Prefilter's s is 1; stored as 0x7BFF
# The bloom family plants HALF_EDGES as twelve constant patches (R = the driver, G = +value, B = -value) that tile the image: columns 0-3, 4-9, 10-15, 16-.. and rows 0-3,
# 4-9, 10-.. .  Where level 0 halves the image exactly (24 x 16: every tap weight is 0.5) the texels (row, col) of HALF_EDGE_TEXELS see one patch only — the border patches
# through clamped indices — and the thirteen-tap sum of equal values v is v again (k v is exact or rounds back: 3 v + v = 4 v), so G and B reach the store unchanged.
HALF_EDGE_EXACT_SIZES = ((24, 16),)
HALF_EDGE_COLS, HALF_EDGE_ROWS = (0, 4, 10, 16), (0, 4, 10)
HALF_EDGE_TEXELS = tuple((r, c) for r in (0, 3, 6) for c in (0, 3, 6, 9))      # of down level 0, in the order of HALF_EDGES

# the thirteen taps of Downsample as (ox, oy)
TAPS13 = ((0, 0), (0, 2), (-2, 0), (2, 0), (0, -2), (-2, 2), (2, 2), (2, -2), (-2, -2), (-1, 1), (1, 1), (1, -1), (-1, -1))


# ---- base images
def _base(family, size):
    W, H = size[:2]
    if family == "bloom":
        return B.input_image((W, H) + BLOOM_DEFAULTS + (BLOOM_MINUS_LODS,))
    return np.ascontiguousarray(P.input_image()[28:28 + H, :W])                # the pseudo-random rows: colours in [-0.25, 2.75)


def _adds(pw, ph):
    glow = P.bloom_image()
    a0 = np.ascontiguousarray(glow[12:12 + ph, 23:23 + pw])
    a1 = np.ascontiguousarray(glow[12:12 + ph, 23:23 + pw][::-1, ::-1]) * f32(0.5); a1[..., 3] = 1.0
    assert a0.shape == (ph, pw, 4) and np.isfinite(a0).all() and (a0[..., :3] > 0).all()
    return a0, a1.astype(f32)


def _spots(W, H, n):
    """n distinct interior texels (row, col), spread by a stride coprime to their number"""
    iw, ih = W - 2, H - 2
    count = iw * ih
    stride = next(s for s in range(5, count) if np.gcd(s, count) == 1)
    assert n <= count
    return [(1 + (k * stride + 2) % count // iw, 1 + (k * stride + 2) % count % iw) for k in range(n)]


def _axis32(n_out, n_src, off=0):
    return B._axis(B._coords(n_out, f32), n_src, off, f32)


def zero_weight_taps(family, size):
    """[(axis, out index, the source index fetched under a weight of exactly 0, the source index fetched under 1 - 0)] of the pass that reads the image: the scaled display
    pass, or bloom's first pass (the chain is sized from the presentation size).  Evaluated with bloom_ref._axis in binary32.  Clamped pairs (both indices equal) are left out."""
    W, H = size[:2]
    ow, oh = (size[2], size[3]) if family == "scaled" else (W // 2, H // 2)
    out = []
    for axis, (n_out, n_src) in (("x", (ow, W)), ("y", (oh, H))):
        i0, i1, a = _axis32(n_out, n_src)
        out += [(axis, int(k), int(i1[k]), int(i0[k])) for k in range(n_out) if a[k] == 0 and i0[k] != i1[k]]
    return out


def scaled_footprint(size, row, col):
    """(ph, pw) bool: the presentation texels whose four taps include source texel (row, col)"""
    W, H, pw, ph = size
    xa, xb, _ = _axis32(pw, W); ya, yb, _ = _axis32(ph, H)
    return (((ya == row) | (yb == row))[:, None]) & (((xa == col) | (xb == col))[None, :])


def down0_footprint(src_size, level_size, row, col):
    """(h0, w0) bool: the texels of down level 0 whose thirteen taps (four texels each) include source texel (row, col)"""
    (W, H), (w0, h0) = src_size, level_size
    m = np.zeros((h0, w0), bool)
    for ox, oy in TAPS13:
        xa, xb, _ = _axis32(w0, W, ox); ya, yb, _ = _axis32(h0, H, oy)
        m |= (((ya == row) | (yb == row))[:, None]) & (((xa == col) | (xb == col))[None, :])
    return m


# ---- the classes: each returns [(target, row, col, (r, g, b) bits)]
def _texel_classes(cls, W, H, base):
    ch = lambda r, c, k, u: tuple(u if j == k else fb(base[r, c, j]) for j in range(3))      # one channel replaced, the others as they were
    one = fb(1.0)
    if cls == "nan":
        s = _spots(W, H, 8)
        vals = [ch(*s[0], 0, QNAN), ch(*s[1], 1, SNAN), ch(*s[2], 2, NEG_NAN), (QNAN,) * 3, (SNAN,) * 3, (NEG_NAN,) * 3, (PAYLOAD_NAN, SNAN, NEG_NAN), ch(*s[7], 1, PAYLOAD_NAN)]
    elif cls in ("pos_inf", "neg_inf"):
        u = POS_INF if cls == "pos_inf" else NEG_INF
        s = _spots(W, H, 4)
        vals = [ch(*s[0], 0, u), ch(*s[1], 1, u), ch(*s[2], 2, u), (u,) * 3]
    elif cls == "inf_pair":
        s = _spots(W, H, 6)
        vals = [(POS_INF, POS_INF, one), (POS_INF, NEG_INF, one), (one, POS_INF, NEG_INF), (NEG_INF, one, POS_INF), (NEG_INF, NEG_INF, fb(0.5)), (POS_INF, fb(0.0), NEG_INF)]
    elif cls == "flt_max":
        s = _spots(W, H, 5)
        m, n = FLT_MAX_BITS, FLT_MAX_BITS | 0x80000000
        vals = [(m,) * 3, ch(*s[1], 0, m), ch(*s[2], 2, m), (n,) * 3, (m, n, one)]
    elif cls == "subnormal32":
        s = _spots(W, H, 5)
        vals = [(0x00000001,) * 3, (0x007FFFFF,) * 3, (0x80000001, 0x807FFFFF, 0x00000001), ch(*s[3], 1, 0x00400000), (0x00000001, fb(0.0), 0x807FFFFF)]
    elif cls == "neg_zero":
        s = _spots(W, H, 4)
        vals = [(NEG_ZERO,) * 3, ch(*s[1], 0, NEG_ZERO), (NEG_ZERO, fb(0.0), NEG_ZERO), (fb(0.0), NEG_ZERO, fb(0.25))]
    elif cls == "negative":
        s = _spots(W, H, 6)
        vals = [(fb(-1.0),) * 3, (fb(-0.5), fb(0.5), fb(-1e-3)), (fb(-1e4),) * 3, ch(*s[3], 2, fb(-65504.0)), (fb(-1e-30), fb(-1e30), fb(2.0)), (fb(-3.0e38), fb(1.0), fb(1.0))]
    elif cls == "half_edges":
        s = _spots(W, H, len(HALF_EDGES))
        vals = [(fb(v), fb(-v), fb(v)) for v, _ in HALF_EDGES]
    elif cls == "edge_texels":
        s = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
        vals = [(QNAN,) * 3, (POS_INF,) * 3, (NEG_INF,) * 3, ch(*s[3], 1, NEG_NAN), ch(*s[4], 0, POS_INF), (NEG_INF, one, POS_INF), (SNAN, one, one), (POS_INF, POS_INF, one)]
    elif cls == "isolated":
        s = [(H // 2, W // 2)]
        vals = [(POS_INF, QNAN, NEG_INF)]
    else:
        raise KeyError(cls)
    return [("img", r, c, v) for (r, c), v in zip(s, vals)]


def _patch(rows, cols, v):
    return [("img", r, c, v) for r in rows for c in cols]


def _planted(family, size, cls, base):
    W, H = size[:2]
    if cls == "zero_weight":
        out = []
        for k, (axis, _, zero, one_) in enumerate(zero_weight_taps(family, size)):
            # +Inf at the texel fetched under the weight 0 (Inf * 0 = NaN), and — two lines further along the other axis — at the one fetched under 1 (Inf stays Inf)
            a, b = (H // 2 - 1 + (k % 2), min(H // 2 + 1 + (k % 2), H - 1)) if axis == "x" else (W // 2 - 1 + (k % 2), min(W // 2 + 1 + (k % 2), W - 1))
            out += [("img", a, zero, (POS_INF,) * 3), ("img", b, one_, (POS_INF,) * 3)] if axis == "x" else [("img", zero, a, (POS_INF,) * 3), ("img", one_, b, (POS_INF,) * 3)]
        return out
    if cls == "overflowing_sum":
        if family == "bloom":                              # every tap of the patch is 2.5e38, finite; the second term of the thirteen-tap sum overflows
            return _patch(range(4, 10), range(4, 10), (fb(2.5e38), fb(2.5e38), fb(-2.5e38)))
        big, half, m, n = fb(2.0e38), fb(1.0e38), FLT_MAX_BITS, FLT_MAX_BITS | 0x80000000
        # (s0, s1, s2): s0 + s1 overflows; (s0 + s1) finite and + s2 overflows; the negative side; +Inf reached first, then a finite term; inf - inf across the channels
        sums = [((m,) * 3, (m,) * 3, (fb(0.0),) * 3), ((big,) * 3, (half,) * 3, (half,) * 3), ((n,) * 3, (n,) * 3, (fb(0.0),) * 3), ((m,) * 3, (m,) * 3, (n,) * 3), ((m, n, fb(1.0)), (m, n, fb(1.0)), (fb(0.0),) * 3)]
        if family == "present":
            out = []
            for (r, c), (s0, s1, s2) in zip(_spots(W, H, len(sums)), sums):
                out += [("img", r, c, s0), ("add0", r, c, s1), ("add1", r, c, s2)]
            return out
        # scaled: the four source texels a presentation texel fetches hold one value, so Sampler0's value there is finite; the added images carry the other terms
        pw, ph = size[2], size[3]
        xa, xb, _ = _axis32(pw, W); ya, yb, _ = _axis32(ph, H)
        out = []
        for k, (s0, s1, s2) in enumerate(sums[1:3]):
            py, px = ph // 2, (1 + k * (pw // 2)) % pw
            s0 = tuple(fb(bf(u) * f32(0.5)) for u in s0) if k else s0          # (-FLT_MAX / 2) + (-FLT_MAX): the filter of equal values may round by an ulp, which must not overflow
            out += _patch(sorted({int(ya[py]), int(yb[py])}), sorted({int(xa[px]), int(xb[px])}), s0) + [("add0", py, px, s1), ("add1", py, px, s2)]
        return out
    if cls == "half_edges" and family == "bloom":
        out = []
        rows = [range(a, b) for a, b in zip(HALF_EDGE_ROWS, HALF_EDGE_ROWS[1:] + (H,))]; cols = [range(a, b) for a, b in zip(HALF_EDGE_COLS, HALF_EDGE_COLS[1:] + (W,))]
        for k, (v, _) in enumerate(HALF_EDGES):
            out += _patch(rows[k // 4], cols[k % 4], (fb(HALF_EDGE_DRIVER), fb(v), fb(-v)))
        return out
    return _texel_classes(cls, W, H, base)


_CASES = {}


def case(family, size, cls):
    key = (family, tuple(size), cls)
    if key not in _CASES:
        assert family in ("present", "bloom", "scaled") and cls in CLASSES
        size = tuple(size)
        img = _base(family, size)
        pw, ph = (size[2], size[3]) if family == "scaled" else size[:2]
        add0, add1 = _adds(pw, ph)
        planted = _planted(family, size, cls, img.copy())
        target = {"img": img, "add0": add0, "add1": add1}
        for t, r, c, v in planted:
            target[t].view(np.uint32)[r, c, :3] = v                                   # by bit pattern: a signalling NaN stays one
        positions = sorted({(r, c) for t, r, c, _ in planted if t == "img"})
        bloom = (HALF_EDGE_BLOOM if cls == "half_edges" else BLOOM_DEFAULTS) + (BLOOM_MINUS_LODS,)
        for a in (img, add0, add1):
            a.setflags(write=False)
        _CASES[key] = Case(family, size, cls, img, add0, add1, tuple(planted), tuple(positions), bloom)
    return _CASES[key]


def table(family, size):
    """{class: [(row, col)]} of the texels planted into the image"""
    return {cls: list(case(family, size, cls).positions) for cls in CLASSES}


def with_zero(c):
    """the image of a case with every planted texel replaced by 0 (the comparison image of the containment checks)"""
    img = c.img.copy()
    for t, r, k, _ in c.planted:
        if t == "img":
            img[r, k, :3] = 0.0
    return img


def bloom_case(c):
    """the bloom_ref case tuple (W, H, Threshold, MaxColor, MinusLods) of a case: the chain is sized from the presentation size"""
    w, h = (c.size[2], c.size[3]) if c.family == "scaled" else c.size[:2]
    return (w, h) + c.bloom
