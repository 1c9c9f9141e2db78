"""Adversarial pixels on the CPU (tests/adversarial_pixels.py): every class is what it claims; the restatements of the display chain (tests/present_ref.py,
tests/present_scaled_ref.py, tests/bloom_ref.py) follow the rule of include/idkpt.h ("Non-finite and extreme texels") and return on every finite input exactly what they
returned before they were brought to it; the host build of the kernels' own texel functions (idkengine_amd/csrc/bloom_texel.hpp through
tests/c_driver/present_scaled_host.cpp, a stand-alone program under ASan/UBSan) equals the restatement on the adversarial images; and the invariants of the rule hold.

presentk (csrc/kernels_present.hpp: AgX_DS, DualSection, quantise) does NOT build for the host: it is written against the device header pt_device.hpp (DEV, f3, gmax /
gmin / gclamp).  So the tone curve has no host build here; its NaN handling is checked on the restatement (np.fmax / np.fmin, the binary32 functions fmaxf / fminf that the
kernel's builtins are) and on the device (tests/test_gpu_adversarial_pixels.py).  The filter and the sum in front of the tone curve — everything the scaled pass adds — do
build for the host and are compared.

Equality throughout: adversarial_pixels.same_value (binary32) and same_half (stored halves); every texel of every array is compared."""
import os
import sys
from unittest import mock
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adversarial_pixels as A  # noqa: E402
import bloom_ref as B  # noqa: E402
import present_ref as P  # noqa: E402
import present_scaled_ref as S  # noqa: E402

f32 = np.float32
FAMILIES = [("present", s) for s in A.PRESENT_SIZES] + [("bloom", s) for s in A.BLOOM_SIZES] + [("scaled", s) for s in A.SCALED_SIZES]
IDS = [f"{f}-{'x'.join(map(str, s))}" for f, s in FAMILIES]
quiet = lambda: np.errstate(all="ignore")                 # Inf * 0 and inf - inf are the subject here, not an accident


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def present_of(c, tm, adds, dtype=f32, img=None):
    """the restatement's display of a case of family present or scaled"""
    img = c.img if img is None else img
    a0, a1 = (c.add0, c.add1) if adds else (None, None)
    with quiet():
        return P.present(img, tm, a0, a1, dtype) if c.family == "present" else S.present_scaled(img, c.size[2], c.size[3], tm, a0, a1, dtype)


def chain_of(c, img=None):
    with quiet():
        return B.chain(c.img if img is None else img, A.bloom_case(c), f32)


# ---- 1. each class is what it claims ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,size", FAMILIES, ids=IDS)
def test_each_class_is_what_it_claims(family, size):
    tab = A.table(family, size)
    assert set(tab) == set(A.CLASSES)
    H, W = size[1], size[0]
    for cls in A.CLASSES:
        c = A.case(family, size, cls)
        assert c.img.shape == (H, W, 4) and c.img.dtype == f32 and (c.img[..., 3] == 1.0).all() and c.add0.shape == c.add1.shape
        targets = {"img": c.img, "add0": c.add0, "add1": c.add1}
        last = {(t, r, k): v for t, r, k, v in c.planted}                         # (a later plant of the same texel wins)
        for (t, r, k), v in last.items():
            assert bits(targets[t])[r, k, :3].tolist() == list(v), (cls, t, r, k)  # read back by bit pattern
        untouched = np.ones((H, W), bool)
        for r, k in c.positions:
            untouched[r, k] = False
        assert (bits(c.img)[untouched] == bits(A._base(family, size))[untouched]).all() and np.isfinite(c.img[untouched]).all()
        planted = np.array([v for t, _, _, v in c.planted if t == "img"], np.uint32).reshape(-1, 3).view(f32)
        pbits = planted.view(np.uint32)
        if cls == "zero_weight":
            check_zero_weight(c)
            continue
        assert len(c.positions) > 0, cls
        if cls == "nan":
            assert np.isnan(planted).any(axis=1).all() and not np.isinf(planted).any() and {A.QNAN, A.SNAN, A.NEG_NAN} <= set(pbits.ravel().tolist())
            assert (np.isnan(planted).sum(axis=1) == 1).any() and np.isnan(planted).all(axis=1).any()          # one channel only, and all three
        elif cls in ("pos_inf", "neg_inf"):
            u = A.POS_INF if cls == "pos_inf" else A.NEG_INF
            assert (pbits == u).any(axis=1).all() and not np.isnan(planted).any() and (pbits == u).all(axis=1).any() and ((pbits == u).sum(axis=1) == 1).any()
        elif cls == "inf_pair":
            assert ((pbits == A.POS_INF).sum(axis=1) == 2).any() and ((pbits == A.POS_INF).any(axis=1) & (pbits == A.NEG_INF).any(axis=1)).any() and not np.isnan(planted).any()
        elif cls == "flt_max":
            assert np.isfinite(planted).all() and (pbits == A.FLT_MAX_BITS).all(axis=1).any() and (pbits == (A.FLT_MAX_BITS | 0x80000000)).any()
        elif cls == "subnormal32":
            sub = ((pbits & 0x7F800000) == 0) & ((pbits & 0x007FFFFF) != 0)
            assert sub.any(axis=1).all() and (pbits == 1).any() and (pbits == 0x007FFFFF).any() and (pbits == 0x80000001).any()
        elif cls == "neg_zero":
            assert (pbits == A.NEG_ZERO).any(axis=1).all() and (pbits == A.NEG_ZERO).all(axis=1).any()
        elif cls == "negative":
            assert (planted < 0).any(axis=1).all() and np.isfinite(planted).all()
        elif cls == "half_edges":
            assert np.isfinite(planted).all() and {A.fb(v) for v, _ in A.HALF_EDGES} | {A.fb(-v) for v, _ in A.HALF_EDGES} <= set(pbits.ravel().tolist())
        elif cls == "edge_texels":
            assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= set(c.positions) and all(r in (0, H - 1) or k in (0, W - 1) for r, k in c.positions)
            assert (~np.isfinite(planted)).any(axis=1).all() and np.isnan(planted).any() and (pbits == A.POS_INF).any() and (pbits == A.NEG_INF).any()
        elif cls == "isolated":
            assert c.positions == ((H // 2, W // 2),) and not np.isfinite(planted).any()
        elif cls == "overflowing_sum":
            check_overflowing_sum(c)
        if cls in A.FINITE_CLASSES or cls == "overflowing_sum":
            assert np.isfinite(c.img).all() and np.isfinite(c.add0).all() and np.isfinite(c.add1).all()


def check_zero_weight(c):
    taps = A.zero_weight_taps(c.family, c.size)
    if (c.family, c.size) in (("bloom", (33, 19)), ("scaled", (9, 5, 15, 7))):
        assert {a for a, *_ in taps} == ({"y"} if c.family == "bloom" else {"x", "y"})       # the sizes that have a weight of exactly 0
    if c.family == "scaled" and c.size != (9, 5, 15, 7) or (c.family, c.size) == ("bloom", (24, 16)):
        assert taps == []                                                                     # x2 and the non-integer ratios: no weight is exactly 0 (nothing to plant)
    W, H = c.size[:2]
    ow, oh = (c.size[2], c.size[3]) if c.family == "scaled" else (W // 2, H // 2)
    inf = np.isposinf(c.img[..., :3]).all(axis=-1)
    assert int(inf.sum()) == len(c.positions) and len(c.positions) == len({p for p in c.positions})
    for axis, out, zero, one in taps:
        n_out, n_src = (ow, W) if axis == "x" else (oh, H)
        i0, i1, a = B._axis(B._coords(n_out, f32), n_src, 0, f32)                            # the weight, evaluated in binary32
        assert a.dtype == f32 and a[out] == 0 and f32(1.0) - a[out] != 0 and i1[out] == zero and i0[out] == one and zero == one + 1
        line = inf[:, zero] if axis == "x" else inf[zero, :]
        other = inf[:, one] if axis == "x" else inf[one, :]
        assert line.any() and other.any()                                                     # +Inf under the weight 0, and at the neighbour under the weight 1
    if c.family == "scaled" and taps:
        # Inf * 0 = NaN in the filtered sum exactly at the presentation texels that fetch a planted texel under the weight 0
        with quiet():
            s = S.sample(c.img, c.size[2], c.size[3])
        assert np.isnan(s).any() and np.isposinf(s).any()


def check_overflowing_sum(c):
    with quiet():
        if c.family == "bloom":
            W, H = c.size
            d = B._downsample(c.img[..., :3].astype(f32), W // 2, H // 2, f32)
            assert np.isposinf(d[..., :2]).any() and np.isneginf(d[..., 2]).any() and np.abs(c.img).max() < 3e38
            return
        s0 = c.img[..., :3] if c.family == "present" else S.sample(c.img, c.size[2], c.size[3])
        first = (f32(0.0) + s0) + c.add0[..., :3]
        total = first + c.add1[..., :3]
    assert np.isfinite(s0).all() and np.isfinite(c.add0).all() and np.isfinite(c.add1).all()
    assert (np.isfinite(first) & np.isinf(total)).any() and np.isposinf(total).any() and np.isneginf(total).any()
    if c.family == "present":
        assert np.isinf(first).any()                                                          # ... and one where s0 + s1 already overflows


def test_half_edges_reach_the_store_of_level_0_unchanged():
    """The value in front of the store of down level 0 is the planted boundary value bit for bit, and the stored half is the one the generator lists."""
    for size in A.HALF_EDGE_EXACT_SIZES:
        c = A.case("bloom", size, "half_edges")
        ch = chain_of(c)
        assert np.isfinite(ch["down_f"][0]).all()
        for (r, k), (v, h) in zip(A.HALF_EDGE_TEXELS, A.HALF_EDGES):
            got = bits(ch["down_f"][0][r, k])
            assert got.tolist() == [A.fb(A.HALF_EDGE_DRIVER), A.fb(v), A.fb(-v)], (r, k, float(v))
            assert ch["down"][0][r, k].tolist() == [0x7BFF, h, h | 0x8000, 0x3C00], (r, k, float(v))
    # the list itself, against the rule applied to the value: toward zero, 65504 beyond, subnormals
    vals = np.array([v for v, _ in A.HALF_EDGES], f32)
    assert B.rtz_half(vals).tolist() == [h for _, h in A.HALF_EDGES] and B.rtz_half(-vals).tolist() == [h | 0x8000 for _, h in A.HALF_EDGES]


# ---- 2. the restatements follow the rule, and are unchanged on finite inputs ----------------------------------------------------------------------------------------------
def _old_prefilter(c, max_color, threshold, dt):
    """bloom_ref._prefilter as it was (np.maximum / np.minimum propagate a NaN)"""
    knee = dt(np.float32(B.KNEE)) if dt is np.float32 else dt(B.KNEE)
    max_color, threshold = dt(np.float32(max_color)), dt(np.float32(threshold))
    c = np.where(c < max_color, c, max_color)
    b = np.maximum(np.maximum(c[..., 0], c[..., 1]), c[..., 2])
    cx, cy, cz = threshold - knee, knee * dt(2.0), dt(0.25) / knee
    rq = np.minimum(np.maximum(b - cx, dt(0.0)), cy)
    rq = (rq * rq) * cz
    s = np.maximum(rq, b - threshold) / np.maximum(b, dt(0.0001))
    return c * s[..., None]


def _old_rtz_half(v):
    """bloom_ref.rtz_half as it was (numpy's payload for a NaN)"""
    v = np.asarray(v)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    b = h.view(np.uint16).copy()
    away = (np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))) & np.isfinite(v)
    b[away] -= 1
    return b


def _as_before():
    """the three modules as they were: NaN-propagating max / min, numpy's half NaN"""
    return [mock.patch.object(np, "fmax", np.maximum), mock.patch.object(np, "fmin", np.minimum), mock.patch.object(B, "_prefilter", _old_prefilter), mock.patch.object(B, "rtz_half", _old_rtz_half)]


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_restatements_return_on_finite_inputs_exactly_what_they_returned_before():
    """Old and new side by side on the fixtures' inputs, binary32 and binary64: bloom_ref.chain on every case, present_ref.present / quantise on every case, the scaled pass
    and its display without the tone curve.  (The committed fixtures hold llvmpipe's results; the existing tests hold the edited restatements to them within the same bounds.)"""
    def run():
        out = []
        for case in B.CASES[:4]:                                                   # (case 4 differs from case 1 in size only)
            for dt in (np.float32, np.float64):
                ch = B.chain(B.input_image(case), case, dt)
                out += ch["down"] + ch["up"] + ch["down_f"] + ch["up_f"] + [ch["expand"]]
        for case in P.CASES:
            img, add = P.case_inputs(case)
            for dt in (np.float32, np.float64):
                out.append(P.present(img, case, add, None, dt))
            out.append(P.quantise(out[-2]))
        pw, ph = S.SIZES[0]
        for c in S.CASE_IDS:
            out.append(S.present_scaled(P.input_image(), pw, ph, P.CASES[c], S.case_add(c, pw, ph), None, np.float32))
        out.append(S.no_tonemap_display(S.sampled_sum(P.input_image(), pw, ph)))
        return out
    new = run()
    patches = _as_before()
    for p in patches:
        p.start()
    try:
        old = run()
    finally:
        for p in patches:
            p.stop()
    assert np.fmax is not np.maximum and len(new) == len(old) > 60
    for k, (a, b) in enumerate(zip(new, old)):
        assert np.isfinite(np.asarray(a, np.float64) if a.dtype.kind == "f" else 0.0).all() and _same_bytes(a, b), k
    # ... and the fixture's own statement about storage still holds for the new rtz_half, on every texel
    fx = B.load_fixture()
    for k in fx.files:
        if k.startswith(("down_f32_", "up_f32_")):
            assert (B.store(fx[k][..., :3]) == fx[k.replace("f32", "bits")]).all(), k


def test_rtz_half_of_non_finite_values_is_the_headers_rule():
    v = np.array([A.QNAN, A.SNAN, A.NEG_NAN, A.PAYLOAD_NAN, 0xFF800001, A.POS_INF, A.NEG_INF, A.FLT_MAX_BITS, A.FLT_MAX_BITS | 0x80000000, A.NEG_ZERO, 1, 0x80000001], np.uint32).view(f32)
    want = [0x7E00, 0x7E00, 0xFE00, 0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF, 0x8000, 0x0000, 0x8000]
    with quiet():
        v64 = v.astype(np.float64)
    assert B.rtz_half(v).tolist() == want and B.rtz_half(v64).tolist() == want
    assert A.same_half(np.array([0x7E00, 0x7C00], np.uint16), np.array([0xFE00, 0x7C00], np.uint16)).all()
    assert not A.same_half(np.array([0x7E00, 0x7C00, 0x7E00, 0x7E01], np.uint16), np.array([0x7C00, 0xFC00, 0x7F00, 0x7E01 ^ 0x8000], np.uint16)).any()


def test_quantise_never_converts_a_nan():
    x = np.array([[A.QNAN, A.NEG_NAN, A.POS_INF, A.fb(1.0)], [A.NEG_INF, A.PAYLOAD_NAN, A.fb(0.5), A.fb(1.0)], [A.fb(-1.0), A.fb(2.0), A.NEG_ZERO, A.fb(1.0)]], np.uint32).view(f32)
    with np.errstate(all="raise"):                        # an integer conversion of a NaN raises here
        q = P.quantise(x)
    assert q.tolist() == [[0, 0, 255, 255], [0, 0, 128, 255], [0, 255, 0, 255]]


# ---- 3. the host build of the kernels' texel functions -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("adversarial_pixels_host")
    return S.build_host(d), d


def assert_chain_equal(got, want, what):
    for chain in ("down", "up"):
        assert len(got[chain]) == len(want[chain]), what
        for l, (g, w) in enumerate(zip(got[chain], want[chain])):
            ok = A.same_half(g, w)
            assert ok.all(), (what, chain, l, np.argwhere(~ok)[:4].tolist())
    ok = A.same_value(got["expand"][..., :3], want["expand"])
    assert ok.all(), (what, "expand", np.argwhere(~ok)[:4].tolist())


@pytest.mark.parametrize("family,size", [fs for fs in FAMILIES if fs[0] != "present"], ids=[i for i, fs in zip(IDS, FAMILIES) if fs[0] != "present"])
def test_host_build_equals_the_restatement_on_every_class(family, size, host):
    """bloom_texel.hpp compiled with g++ under ASan/UBSan (a stand-alone program): every level of both chains, the expanded image and — at the scaled sizes — the filtered
    sum in front of the tone curve, without and with the added images, for every class."""
    exe, d = host
    for cls in A.CLASSES:
        c = A.case(family, size, cls)
        W, H = size[:2]
        pw, ph = (size[2], size[3]) if family == "scaled" else (W, H)
        got = S.host_bloom(exe, d, c.img, pw, ph, c.bloom)
        assert got["same"] == 1, (cls, "the staged and the direct route of down pass 0 differ")
        assert_chain_equal(got, chain_of(c), (family, size, cls))
        if family == "scaled":
            for adds in ((), (c.add0, c.add1)):
                with quiet():
                    want = S.sampled_sum(c.img, pw, ph, *(adds or (None, None)))
                ok = A.same_value(S.host_sum(exe, d, c.img, pw, ph, adds), want)
                assert ok.all(), (cls, len(adds), np.argwhere(~ok)[:4].tolist())


# ---- 4. invariants of the rule, on the restatement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,size", [fs for fs in FAMILIES if fs[0] != "bloom"], ids=[i for i, fs in zip(IDS, FAMILIES) if fs[0] != "bloom"])
def test_every_present_texel_is_finite_and_bytes_are_the_quantised_floats(family, size):
    for cls in A.CLASSES:
        c = A.case(family, size, cls)
        for tm in A.TONEMAPS:
            for adds in (False, True):
                out = present_of(c, tm, adds)
                assert out.dtype == f32 and np.isfinite(out).all() and (out[..., 3] == 1.0).all(), (cls, tm, adds)
                with np.errstate(all="raise"):
                    q = P.quantise(out)
                # an independent statement of the rule: clip, one binary32 product, round to nearest even through the 2^23 trick (exact for 0 <= x <= 255)
                x = np.clip(out[..., :3], f32(0.0), f32(1.0)) * f32(255.0)
                want = ((x + f32(8388608.0)) - f32(8388608.0)).astype(np.int64)
                assert x.dtype == f32 and (q[..., :3] == want).all() and (q[..., 3] == 255).all()


def test_nan_and_negative_inputs_act_as_zero_in_the_display_pass():
    """max(.., 0) and clamp drop a NaN: a texel whose channels are NaN, -Inf or negative displays exactly what a texel of zeros displays (no added images)."""
    for size in A.PRESENT_SIZES:
        for cls in ("nan", "neg_inf", "negative", "neg_zero"):
            c = A.case("present", size, cls)
            zero = c.img.copy()
            bad = ~(c.img[..., :3] > 0)                   # NaN, negative, -0, 0
            zero[..., :3][bad] = 0.0
            for tm in A.TONEMAPS:
                assert _same_bytes(present_of(c, tm, False), present_of(c, tm, False, img=zero)), (size, cls, tm)


@pytest.mark.parametrize("family,size", FAMILIES, ids=IDS)
def test_an_isolated_texel_changes_only_what_fetches_it(family, size):
    """k_present: its own texel.  The scaled pass: the texels whose four taps include it.  Bloom level 0: the texels whose thirteen-tap footprint includes it.  Outside those
    sets the output equals that of the image with the texel replaced by 0, bit for bit."""
    c = A.case(family, size, "isolated")
    (r, k), = c.positions
    zero = A.with_zero(c)
    if family == "bloom":
        a, b = chain_of(c), chain_of(c, img=zero)
        w0, h0 = size[0] // 2, size[1] // 2
        inside = A.down0_footprint(size, (w0, h0), r, k)
        changed = (a["down"][0] != b["down"][0]).any(axis=-1)
        assert 0 < inside.sum() < inside.size and not (changed & ~inside).any() and changed.any()
        assert (bits(a["down_f"][0])[~inside] == bits(b["down_f"][0])[~inside]).all()
        return
    for tm in A.TONEMAPS:
        for adds in (False, True):
            a, b = present_of(c, tm, adds), present_of(c, tm, adds, img=zero)
            inside = np.zeros(a.shape[:2], bool)
            if family == "present":
                inside[r, k] = True
            else:
                inside = A.scaled_footprint(size, r, k)
            changed = (bits(a) != bits(b)).any(axis=-1)
            assert 0 < inside.sum() < inside.size and changed.any() and not (changed & ~inside).any(), (tm, adds)
            if family == "scaled":
                bs = chain_of(c); bz = chain_of(c, img=zero)
                lv = (size[2] // 2, size[3] // 2)
                fp = A.down0_footprint(size[:2], lv, r, k)
                assert not ((bs["down"][0] != bz["down"][0]).any(axis=-1) & ~fp).any()
