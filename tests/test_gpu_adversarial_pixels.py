"""Adversarial pixels on the device (tests/adversarial_pixels.py): idkptPresent, idkptBloom and the display chain at a presentation size on NaN, +-Inf, FLT_MAX, overflowing
sums, binary32 subnormals, -0, negatives and the half-precision boundaries — every class, every size, both display formats, with and without the added images — against
the restatements (tests/present_ref.py, tests/present_scaled_ref.py, tests/bloom_ref.py) under the rule of include/idkpt.h ("Non-finite and extreme texels").

What is compared how, at every texel:
  * Bloom (every level of both chains, the expanded image) and the displays WITHOUT the tone curve (DoTonemapAndSrgbTransform = 0: filter, sum, clamp, dither): the equality
    of adversarial_pixels — equal bits, or both NaN (stored halves: both sign | 0x7E00), or the same signed infinity.  Nothing there is implementation-defined.
  * Displays WITH the tone curve: every texel finite, and held in the project's measured-bound form (tests/test_present_ref.py), because expf (DualSection) and powf
    (LinearToSrgb) are library functions and differ between the device and numpy, so bits cannot be equal.  Per case (size, settings, added images), from the
    llvmpipe fixture tests/golden/adversarial_pixels/present.npz and the binary64 value T of the formula: b = 2 x max(e_gl, e_np), measured over the texels no planted
    texel reaches (tests/test_adversarial_pixels_glref.py touched()) of the thirteen images of that size; there |device - T| <= b.  On the texels a planted texel reaches binary64 is no yardstick (binary32
    overflows where it does not, and GLSL leaves the NaN undefined): the rule's statement there is the binary32 restatement, which lies within e_np of the exact value of its
    own operation sequence while the device lies within b of it, so |device - restatement| <= b + e_np.  b is 1e-6 .. 5e-6; a NaN or an infinity handled otherwise than the
    rule says moves a texel by the whole range.  Every figure is printed (profiles/display_nonfinite.md records them).
  * RGBA8 equals present_ref.quantise of the device's own RGBA32F, bit for bit; the guard bytes behind the image are intact."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import adversarial_pixels as A  # noqa: E402
import adversarial_surfaces as AS  # noqa: E402
import bloom_ref as B  # noqa: E402
import present_ref as P  # noqa: E402
import present_scaled_ref as S  # noqa: E402
import test_adversarial_pixels_glref as G  # noqa: E402
from test_present_ref import present_bound  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from test_gpu_present import same, settings_of, write_result, c_present, c_download, c_device_display, plain_pt, GUARD  # noqa: E402
from test_gpu_bloom import c_bloom, c_info, c_level, c_expanded  # noqa: E402
from test_gpu_present_scaled import set_pres, download, device_display, expanded, to_device, route  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
RGBA8, RGBA32F = T.IDKPT_DISPLAY_RGBA8, T.IDKPT_DISPLAY_RGBA32F
FX = np.load(os.path.join(G.DIR, "present.npz"))
quiet = lambda: np.errstate(all="ignore")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


_POOLED = {}


def tone_bound(c, t, adds):
    """(b, e_gl, e_np, binary64 value, touched) of a case of family present / scaled under A.TONEMAPS[t], from the llvmpipe fixture.  e_gl and e_np are the largest over the
    thirteen images of the case's size (the same arithmetic and settings on the same background; an image of 45 texels alone is too small a sample of exp's and pow's
    rounding: its own largest error can be a third of its neighbour's)."""
    key = (c.family, c.size, t, int(adds))
    if key not in _POOLED:
        e_gl = e_np = 0.0
        for i, cls in enumerate(A.CLASSES):
            k = A.case(c.family, c.size, cls)
            fx = FX[f"p_{c.family}_{G.size_id(c.size)}_f32"][i, t, int(adds)]
            r32, r64 = G.restated_display(k, A.TONEMAPS[t], adds, f32), G.restated_display(k, A.TONEMAPS[t], adds, np.float64)
            m = G.touched(k)
            if not (~m).any():                             # (a planted border reaches every texel of a 7 x 5 display)
                continue
            _, g, n = present_bound(fx[~m], r32[~m], r64[~m])
            e_gl, e_np = max(e_gl, g), max(e_np, n)
        _POOLED[key] = (2.0 * max(e_gl, e_np), e_gl, e_np)
    b, e_gl, e_np = _POOLED[key]
    return b, e_gl, e_np, G.restated_display(c, A.TONEMAPS[t], adds, np.float64), G.touched(c)


def hold_display(got, want, tm, what, bound=None):
    """a device RGBA32F display against the restatement's, by the module's rule; bound = tone_bound(..) for a display with the tone curve"""
    assert got.dtype == f32 and got.shape == want.shape and np.isfinite(got).all() and (got[..., 3] == 1.0).all(), what
    if int(tm[5]):
        b, e_gl, e_np, r64, m = bound
        e_out = P.err(got[~m], r64[~m]) if (~m).any() else 0.0
        e_in = float(np.abs(got.astype(np.float64) - want.astype(np.float64))[m].max()) if m.any() else 0.0
        print(f"{what}: e_gl = {e_gl:.3e}  e_np = {e_np:.3e}  bound = {b:.3e}  e_device = {e_out:.3e}  |device - restatement| on reached texels = {e_in:.3e}")
        assert 0.0 < b < 1.0 / 510.0 and e_out <= b and e_in <= b + e_np, (what, e_out, e_in, b)
    else:
        ok = A.same_value(got, want)
        assert ok.all(), (what, np.argwhere(~ok)[:4].tolist())


def hold_chain(pt, want, what, slot=-1):
    """every level of both chains and the expanded image of the slot's bloom against a bloom_ref.chain"""
    levels, w0, h0 = c_info(pt, slot)
    assert levels == len(want["down"]) and (h0, w0) == want["down"][0].shape[:2], what
    got = dict(down=[c_level(pt, 0, l, slot) for l in range(levels)], up=[c_level(pt, 1, l, slot) for l in range(levels - 1)])
    for chain in ("down", "up"):
        for l, (g, w) in enumerate(zip(got[chain], want[chain])):
            ok = A.same_half(g, w)
            assert (g[..., 3] == 0x3C00).all() and ok.all(), (what, chain, l, np.argwhere(~ok)[:4].tolist())
    return got


def present_both(pt, c, t, adds, dev_adds, want, what, size):
    """RGBA32F held to `want`; RGBA8 = quantise(own RGBA32F); guards intact.  size = (pw, ph) of the display"""
    pw, ph = size
    tm = A.TONEMAPS[t]
    kw = dict(add0=dev_adds[0].data_ptr(), add1=dev_adds[1].data_ptr()) if adds else {}
    st = settings_of(tm)
    pt._check(c_present(pt, st, RGBA32F, **kw))
    d32, g32 = device_display(pt, RGBA32F, pw, ph)
    d32 = d32.copy()
    assert same(download(pt, RGBA32F, pw, ph), d32) and (g32 == 0xA5).all() and len(g32) == GUARD, what
    hold_display(d32, want, tm, what, tone_bound(c, t, adds) if int(tm[5]) else None)
    pt._check(c_present(pt, st, RGBA8, **kw))
    d8, g8 = device_display(pt, RGBA8, pw, ph)
    assert same(d8.copy(), P.quantise(d32)) and (d8[..., 3] == 255).all() and (g8 == 0xA5).all() and len(g8) == GUARD, what
    return d32


@pytest.mark.parametrize("size", A.PRESENT_SIZES, ids=[f"{w}x{h}" for w, h in A.PRESENT_SIZES])
def test_present_on_every_class(size):
    """idkptPresent (k_present): 9 x 5 (the W mod 4 row tail) and 16 x 8 (the full 16-byte store); the three tone settings; without and with dAdd0 / dAdd1."""
    W, H = size
    pt = plain_pt(W, H)
    for cls in A.CLASSES:
        c = A.case("present", size, cls)
        write_result(pt, c.img)
        dev_adds = (to_device(c.add0), to_device(c.add1))
        for t, tm in enumerate(A.TONEMAPS):
            for adds in (False, True):
                with quiet():
                    want = P.present(c.img, tm, c.add0 if adds else None, c.add1 if adds else None, f32)
                d32 = present_both(pt, c, t, adds, dev_adds, want, f"present {W}x{H} {cls} tonemap {tm[5]} linear {tm[2]} adds {adds}", size)
                if cls == "isolated":                      # containment, recomputed from the device's output: only the texel itself differs from the image with a 0 there
                    (r, k), = c.positions
                    write_result(pt, A.with_zero(c))
                    kw = dict(add0=dev_adds[0].data_ptr(), add1=dev_adds[1].data_ptr()) if adds else {}
                    pt._check(c_present(pt, settings_of(tm), RGBA32F, **kw))
                    changed = (bits(c_download(pt, RGBA32F)) != bits(d32)).any(axis=-1)
                    changed[r, k] = False
                    assert not changed.any(), (tm, adds)
                    write_result(pt, c.img)
    pt.Dispose()


@pytest.mark.parametrize("size", A.BLOOM_SIZES, ids=[f"{w}x{h}" for w, h in A.BLOOM_SIZES])
def test_bloom_on_every_class(size):
    """idkptBloom: every down and up level's half bits and the expanded image equal bloom_ref.chain(.., float32); half_edges land on the half bit patterns the generator lists;
    an isolated texel changes level 0 only inside its thirteen-tap footprint."""
    W, H = size
    pt = plain_pt(W, H)
    for cls in A.CLASSES:
        c = A.case("bloom", size, cls)
        with quiet():
            want = B.chain(c.img, A.bloom_case(c), f32)
        write_result(pt, c.img)
        pt._check(c_bloom(pt, T.BloomSettings(*c.bloom)))
        got = hold_chain(pt, want, f"bloom {W}x{H} {cls}")
        body, guard, _ = c_expanded(pt, extra=GUARD)
        ok = A.same_value(body[..., :3], want["expand"])
        assert ok.all() and (body[..., 3] == 1.0).all() and (guard == 0xA5).all(), (cls, np.argwhere(~ok)[:4].tolist())
        if cls == "half_edges" and size in A.HALF_EDGE_EXACT_SIZES:
            for (r, k), (v, h) in zip(A.HALF_EDGE_TEXELS, A.HALF_EDGES):
                assert got["down"][0][r, k].tolist() == [0x7BFF, h, h | 0x8000, 0x3C00], (r, k, float(v))
        if cls == "isolated":
            (r, k), = c.positions
            write_result(pt, A.with_zero(c))
            pt._check(c_bloom(pt, T.BloomSettings(*c.bloom)))
            changed = (c_level(pt, 0, 0) != got["down"][0]).any(axis=-1)
            inside = A.down0_footprint(size, (W // 2, H // 2), r, k)
            assert changed.any() and not (changed & ~inside).any()
    pt.Dispose()


@pytest.mark.parametrize("size", A.SCALED_SIZES, ids=["{}x{}_at_{}x{}".format(*s) for s in A.SCALED_SIZES])
def test_scaled_present_and_bloom_on_every_class(size):
    """idkptSetPresentationSize: k_present_scaled against present_scaled_ref, bloom's first pass (k_bloom_down0, and k_bloom_down0_direct when supersampling) and the rest
    of the chain against bloom_ref with the chain sized from the presentation size; an isolated texel reaches only the texels whose taps include it."""
    W, H, pw, ph = size
    pt = plain_pt(W, H)
    assert set_pres(pt, pw, ph) == 0
    for cls in A.CLASSES:
        c = A.case("scaled", size, cls)
        write_result(pt, c.img)
        dev_adds = (to_device(c.add0), to_device(c.add1))
        shown = {}
        for t, tm in enumerate(A.TONEMAPS):
            for adds in (False, True):
                with quiet():
                    want = S.present_scaled(c.img, pw, ph, tm, c.add0 if adds else None, c.add1 if adds else None, f32)
                shown[tm, adds] = present_both(pt, c, t, adds, dev_adds, want, f"scaled {size} {cls} tonemap {tm[5]} adds {adds}", (pw, ph))
        with quiet():
            want = B.chain(c.img, A.bloom_case(c), f32)
        pt._check(c_bloom(pt, T.BloomSettings(*c.bloom)))
        assert route(pt) == (T.IDKPT_BLOOM_ROUTE_DIRECT if size in A.DIRECT_ROUTE_SIZES else T.IDKPT_BLOOM_ROUTE_TILED)
        got = hold_chain(pt, want, f"scaled bloom {size} {cls}")
        body, guard, _ = expanded(pt, pw, ph)
        ok = A.same_value(body[..., :3], want["expand"])
        assert ok.all() and (guard == 0xA5).all(), (cls, np.argwhere(~ok)[:4].tolist())
        if cls == "isolated":
            (r, k), = c.positions
            write_result(pt, A.with_zero(c))
            inside = A.scaled_footprint(size, r, k)
            for (tm, adds), d32 in shown.items():
                kw = dict(add0=dev_adds[0].data_ptr(), add1=dev_adds[1].data_ptr()) if adds else {}
                pt._check(c_present(pt, settings_of(tm), RGBA32F, **kw))
                changed = (bits(download(pt, RGBA32F, pw, ph)) != bits(d32)).any(axis=-1)
                assert 0 < inside.sum() < inside.size and not (changed & ~inside).any(), (tm, adds)
            pt._check(c_bloom(pt, T.BloomSettings(*c.bloom)))
            changed = (c_level(pt, 0, 0) != got["down"][0]).any(axis=-1)
            assert not (changed & ~A.down0_footprint((W, H), (pw // 2, ph // 2), r, k)).any()
    pt.Dispose()


def test_a_rendered_non_finite_frame_is_displayed_as_the_restatements_say(native_builder):
    """End to end: one 16 x 16 frame of adversarial_surfaces' non_finite room (two accumulated samples: inf, then inf * 0) from the path tracer, bloomed and presented at the
    render size.  Result really holds an Inf and a NaN; the bloom equals bloom_ref.chain of the downloaded Result; the display bytes without the tone curve equal the
    restatements applied to that Result bit for bit, with the tone curve they are the quantised floats, which are held to the restatement's."""
    from idkengine_amd.pathtracer import PathTracer
    w = h = 16
    sc = AS.cached_room("non_finite", native_builder); pf = AS.camera("A", w, h)
    pt = PathTracer(w, h, settings=T.Settings.default())
    pt.UploadScene(sc); pt.SetPerFrameData(pf)
    pt.Compute(); pt.Compute()
    result = pt.Result
    assert np.isinf(result[..., :3]).any() and np.isnan(result[..., :3]).any()
    bloom = (1.5, 3.8, 1)
    with quiet():
        want = B.chain(result, (w, h) + bloom, f32)
    pt._check(c_bloom(pt, T.BloomSettings(*bloom)))
    hold_chain(pt, want, "rendered frame")
    body, _, ptr = c_expanded(pt, extra=GUARD)
    assert A.same_value(body[..., :3], want["expand"]).all()
    glow = np.ones((h, w, 4), f32); glow[..., :3] = body[..., :3]
    everywhere = np.ones((h, w), bool)                       # the glow of a frame that holds Inf and NaN reaches every texel: all of them are "reached"
    for t, tm in enumerate(A.TONEMAPS):
        with quiet():
            ref = P.present(result, tm, glow, None, f32)
        pt._check(c_present(pt, settings_of(tm), RGBA32F, add0=ptr)); d32 = c_download(pt, RGBA32F)
        # no fixture of a rendered frame: the bound of the same settings measured on the 16 x 8 fixture case with added images
        b, e_gl, e_np, _, _ = tone_bound(A.case("present", (16, 8), "isolated"), t, True) if int(tm[5]) else (None,) * 5
        hold_display(d32, ref, tm, f"rendered frame tonemap {tm[5]} linear {tm[2]}", (b, e_gl, e_np, None, everywhere))
        pt._check(c_present(pt, settings_of(tm), RGBA8, add0=ptr)); d8 = c_download(pt, RGBA8)
        assert same(d8, P.quantise(d32))
        if not int(tm[5]):
            assert same(d8, P.quantise(ref))
    pt.Dispose()
