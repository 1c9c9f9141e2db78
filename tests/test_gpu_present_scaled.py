"""The display chain at a presentation size other than the render size, on the device: idkptSetPresentationSize / idkptGetPresentationSize, the scaled idkptPresent
(csrc/kernels_present.hpp k_present_scaled) and the scaled idkptBloom (csrc/host_bloom.hpp; k_bloom_down0 reading the smaller image, k_bloom_down0_direct for
supersampling, k_bloom_expand at the presentation size).

Held to what tests/test_present_scaled_ref.py establishes on the CPU: floats within the case's bound (2 x the larger error of the two binary32 executions of the reference
material against the binary64 value, computed from the fixture at run time) of the binary64 value; bytes equal to the quantised binary64 value, one step off only within the
bound of a rounding tie; and bit for bit wherever no exp / pow is involved (see that file's docstring for why the tone curve cannot be): the filtered sum in front of the tone
curve against the host build of the same filter (tests/c_driver/present_scaled_host.cpp) through the displays of DoTonemapAndSrgbTransform = 0, every bloom level and the
expanded image against the restatement and the host build, equal sizes against today's kernels, accumulation, ring slots, guards, tails, failures, the Python layer.
The filtered sum is compared bit for bit over its whole range, HDR and negative values included: the filter is exact under a power-of-two scale and a sign change (asserted for
the host build in tests/test_present_scaled_ref.py), so the input is presented at scales 2^k and with both signs until every texel has been seen inside [0, 1], in front of
the clamp."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import bloom_ref as B  # noqa: E402
import present_ref as P  # noqa: E402
import present_scaled_ref as R  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from test_gpu_present import same, settings_of, write_result, read_device, c_present, plain_pt  # noqa: E402
from test_gpu_bloom import c_bloom, c_info, c_level  # noqa: E402

pytestmark = pytest.mark.gpu
W, H = P.W, P.H
INVALID_ARGUMENT, INVALID_OPERATION = 2, 3
RGBA8, RGBA32F = T.IDKPT_DISPLAY_RGBA8, T.IDKPT_DISPLAY_RGBA32F
GUARD = 64
OFF = T.TonemapSettings(DoTonemapAndSrgbTransform=False)


def set_pres(pt, w, h):
    return pt._L.idkptSetPresentationSize(pt._ctx, w, h)


def get_pres(pt):
    w, h = C.c_int32(), C.c_int32()
    pt._check(pt._L.idkptGetPresentationSize(pt._ctx, C.byref(w), C.byref(h)))
    return w.value, h.value


def last_error(pt):
    msg = C.c_char_p()
    pt._L.idkptGetLastError(pt._ctx, C.byref(msg))
    return (msg.value or b"").decode()


def download(pt, fmt, pw, ph, slot=-1):
    out = np.zeros((ph, pw, 4), np.float32 if fmt == RGBA32F else np.uint8)
    pt._check(pt._L.idkptDownloadDisplay(pt._ctx, slot, out.ctypes.data, out.nbytes))
    return out


def display(pt, tm, fmt, pw, ph, **kw):
    pt._check(c_present(pt, tm, fmt, **kw))
    return download(pt, fmt, pw, ph, kw.get("slot", -1))


def device_display(pt, fmt, pw, ph, slot=-1):
    """(image, guard) through idkptGetDisplayDevicePtr"""
    p = C.c_void_p(); n = C.c_size_t()
    pt._check(pt._L.idkptGetDisplayDevicePtr(pt._ctx, slot, C.byref(p), C.byref(n)))
    assert n.value == ph * pw * (16 if fmt == RGBA32F else 4)
    raw = read_device(pt, p.value, n.value + GUARD)
    return raw[:n.value].view(np.float32 if fmt == RGBA32F else np.uint8).reshape(ph, pw, 4), raw[n.value:]


def expanded(pt, pw, ph, slot=-1):
    """(image, guard, pointer) of idkptGetBloomDevicePtr"""
    p = C.c_void_p(); n = C.c_size_t()
    pt._check(pt._L.idkptGetBloomDevicePtr(pt._ctx, slot, C.byref(p), C.byref(n)))
    assert n.value == ph * pw * 16
    raw = read_device(pt, p.value, n.value + GUARD)
    return raw[:n.value].view(np.float32).reshape(ph, pw, 4), raw[n.value:], p.value


def chain_with_guard(pt, chain, slot=-1):
    """(the chain's bytes, its guard) through idkptGetBloomChainDevicePtr"""
    p = C.c_void_p(); n = C.c_size_t()
    pt._check(pt._L.idkptGetBloomChainDevicePtr(pt._ctx, slot, chain, C.byref(p), C.byref(n)))
    raw = read_device(pt, p.value, n.value + GUARD)
    return raw[:n.value], raw[n.value:]


def route(pt, slot=-1):
    r = C.c_int32(-1)
    pt._check(pt._L.idkptGetBloomRoute(pt._ctx, slot, C.byref(r)))
    return r.value


def to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda")
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("present_scaled_host")
    return R.build_host(d), d


@pytest.fixture(scope="module")
def fixture():
    return np.load(R.FIXTURE)


@pytest.fixture(scope="module")
def bloom_fx():
    return np.load(R.BLOOM_FIXTURE)


GROUPS = [f"{pw}x{ph}" for pw, ph in R.SIZES] + ["small"]


@pytest.mark.parametrize("group", GROUPS)
def test_every_size_and_case_in_both_formats(group, fixture, host):
    """1. Floats within the case's bound of binary64; bytes the quantised binary64 value, off by 1 only within the bound of a tie; the device's bytes are the header's
    quantisation of its own floats; and the displays without the tone curve equal the host build's filtered sum (clamped, dithered) bit for bit — without and with Sampler1."""
    exe, d = host
    entries = [e for e in R.entries() if e[0].rsplit("_", 1)[0] == group]
    assert entries
    img, (pw, ph) = entries[0][1], entries[0][2]
    pt = plain_pt(img.shape[1], img.shape[0])
    write_result(pt, img)
    assert set_pres(pt, pw, ph) == 0 and get_pres(pt) == (pw, ph)
    glow = R.bloom_image(pw, ph); d_glow = to_device(glow)
    for key, _, _, c in entries:
        case, add = P.CASES[c], (glow if P.CASES[c][6] else None)
        f32, f64 = R.present_scaled(img, pw, ph, case, add, None, np.float32), R.present_scaled(img, pw, ph, case, add, None, np.float64)
        rows, fx, by = R.fixture_entry(fixture, key, pw, ph)
        bound = max(R.bound_of(fx, f32[rows], f64[rows])[0], 2.0 * P.err(f32, f64))
        kw = dict(add0=d_glow.data_ptr()) if add is not None else {}
        got = display(pt, settings_of(case), RGBA32F, pw, ph, **kw)
        got8 = display(pt, settings_of(case), RGBA8, pw, ph, **kw)
        e_dev = P.err(got, f64)
        print(f"{key}: e_device = {e_dev:.3e}  bound = {bound:.3e}  texels equal to the restatement bit for bit: {float((got.view(np.uint32) == f32.view(np.uint32)).all(-1).mean()):.3f}")
        assert 0.0 < bound < 1.0 / 510.0 and e_dev <= bound, (key, e_dev, bound)
        assert (got[..., 3] == 1.0).all() and same(got8, P.quantise(got))
        x = np.minimum(np.maximum(f64[..., :3], 0.0), 1.0) * 255.0
        q64 = np.rint(x).astype(np.int64); step = np.abs(got8[..., :3].astype(np.int64) - q64)
        near_tie = np.abs((x - np.floor(x)) - 0.5) <= bound * 255.0
        assert step.max() <= 1 and not ((step == 1) & ~near_tie).any() and (got8[..., 3] == 255).all(), key
        assert P.err(fx, f64[rows]) <= bound
    # in front of the tone curve: bit for bit with the host build of the same filter
    want = R.no_tonemap_display(R.host_sum(exe, d, img, pw, ph))
    assert same(display(pt, OFF, RGBA32F, pw, ph), want) and same(display(pt, OFF, RGBA8, pw, ph), P.quantise(want))
    want = R.no_tonemap_display(R.host_sum(exe, d, img, pw, ph, (glow,)))
    assert same(display(pt, OFF, RGBA32F, pw, ph, add0=d_glow.data_ptr()), want)
    want = R.no_tonemap_display(R.host_sum(exe, d, img, pw, ph, (glow, glow[::-1].copy())))
    d_flip = to_device(glow[::-1].copy())
    assert same(display(pt, OFF, RGBA32F, pw, ph, add0=d_glow.data_ptr(), add1=d_flip.data_ptr()), want)
    body, guard = device_display(pt, RGBA32F, pw, ph)
    assert same(body, want) and len(guard) == GUARD and (guard == 0xA5).all()
    # ... over the whole range of the sum, not only where it lies in [0, 1]: scaled by powers of two and negated (both exact in the filter), every texel in front of the clamp
    hsum = R.host_sum(exe, d, img, pw, ph)
    seen = np.zeros(hsum.shape, bool)
    for k in R.SCALE_EXPONENTS:
        for sign in (1.0, -1.0):
            sc = np.float32(sign * 2.0 ** k)
            scaled = img.copy(); scaled[..., :3] *= sc
            write_result(pt, scaled)
            hs = hsum * sc + np.float32(0.0)                            # == host_sum(scaled) bit for bit (test_present_scaled_ref.py; 0 + (-0) = +0)
            assert same(display(pt, OFF, RGBA32F, pw, ph), R.no_tonemap_display(hs)), (k, sign)
            seen |= (hs >= 2.0 ** -4) & (hs <= 1.0)
    assert (seen | (np.abs(hsum) < 2.0 ** -18)).all()                   # every value of magnitude >= 2^-18 was compared inside [2^-4, 1]: at most 3 of its low bits under the dither's rounding
    pt.Dispose()


@pytest.mark.parametrize("c", range(len(R.BLOOM_CHAINS)))
def test_bloom_chain_sized_from_the_presentation_size(c, bloom_fx, host):
    """2. Every level of both chains and the expanded image: the restatement and the host build bit for bit; the fixture by the per-pass rule rtz(T - b) <= h <= rtz(T + b) with
    T the binary64 evaluation of the pass from the device's own input levels.  23 x 13 from 70 x 40 takes the direct-fetch route (the stat and the result)."""
    exe, d = host
    Ws, Hs, pw, ph = R.BLOOM_CHAINS[c]
    thr, maxc, minus = R.BLOOM_SETTINGS
    img = R.bloom_source(Ws, Hs)
    pt = plain_pt(Ws, Hs)
    write_result(pt, img)
    assert set_pres(pt, pw, ph) == 0
    bs = T.BloomSettings(thr, maxc, minus)
    pt._check(c_bloom(pt, bs))
    levels, sz = B.sizes(pw, ph, minus)
    assert c_info(pt) == (levels, sz[0][0], sz[0][1])
    assert route(pt) == (T.IDKPT_BLOOM_ROUTE_DIRECT if c == 2 else T.IDKPT_BLOOM_ROUTE_TILED)
    down = [c_level(pt, 0, l) for l in range(levels)]; up = [c_level(pt, 1, l) for l in range(levels - 1)]
    ex, guard, _ = expanded(pt, pw, ph)
    want, hostc = R.bloom_chain(img, pw, ph, np.float32), R.host_bloom(exe, d, img, pw, ph)
    assert hostc["same"] == 1
    for l in range(levels):
        assert same(down[l], want["down"][l]) and same(down[l], hostc["down"][l]), (c, "down", l)
    for l in range(levels - 1):
        assert same(up[l], want["up"][l]) and same(up[l], hostc["up"][l]), (c, "up", l)
    assert same(np.ascontiguousarray(ex[..., :3]), want["expand"]) and same(ex, hostc["expand"]) and (ex[..., 3] == 1.0).all()
    assert len(guard) == GUARD and (guard == 0xA5).all()
    # the chains as they lie in memory: the levels one behind the other, and 64 bytes of 0xA5 behind each chain that no pass — the direct-fetch one included — wrote
    for chain, lv in ((0, down), (1, up)):
        body, cguard = chain_with_guard(pt, chain)
        assert body.tobytes() == b"".join(l.tobytes() for l in lv), (c, chain)
        assert len(cguard) == GUARD and (cguard == 0xA5).all(), (c, chain)
    # the fixture, pass by pass
    for name, chain, l, bits, f32, np32, np64 in R.bloom_passes(bloom_fx, c):
        b, _, _ = R.bound_of(f32, np32, np64, B.err)
        if chain == "down":
            T64 = B.down_pass0(img, sz[0], thr, maxc, np.float64) if l == 0 else B.down_pass(down[l - 1], sz[l], np.float64, (thr, maxc) if l == 1 else None)
            got = down[l]
        else:
            T64 = B.up_pass(down[l + 1] if l == levels - 2 else up[l + 1], down[l + 1], sz[l], np.float64)
            got = up[l]
        assert R.halves_within(got, T64, b).all(), (c, name)
    e32, e64 = B.expand(bloom_fx[f"up_bits_{c}_0"], pw, ph, np.float32), B.expand(bloom_fx[f"up_bits_{c}_0"], pw, ph, np.float64)
    b, _, _ = R.bound_of(bloom_fx[f"expand_{c}"], e32, e64, B.err)
    assert B.err(ex, B.expand(up[0], pw, ph, np.float64)) <= b
    # a second bloom gives the same bits
    pt._check(c_bloom(pt, bs))
    assert same(c_level(pt, 0, 0), down[0])
    pt.Dispose()


def test_dither_phase_is_the_presentation_texels():
    """3. Constant grey, DoTonemapAndSrgbTransform = 0, 93 x 53 from 70 x 40: 0.5 + d[x % 8, y % 8] exactly (every filter weight pair sums a constant to itself)."""
    pt = plain_pt()
    write_result(pt, np.full((H, W, 4), 0.5, np.float32))
    assert set_pres(pt, 93, 53) == 0
    got = display(pt, OFF, RGBA32F, 93, 53)
    dth = P.dither_values(np.float32)
    want = np.float32(0.5) + dth[(np.arange(93) % 8)[None, :], (np.arange(53) % 8)[:, None]]
    for ch in range(3):
        assert same(np.ascontiguousarray(got[..., ch]), want)
    pt.Dispose()


@pytest.mark.parametrize("pw", [92, 93, 94, 95])
def test_width_tails(pw, host):
    """4. pw mod 4 in {0, 1, 2, 3} at 5 rows: the 16-byte stores and the texel-wise tail give the header's quantisation of the RGBA32F display (one float4 per texel), which is
    the host build's; the guard behind both buffers stays 0xA5."""
    exe, d = host
    ph = 5
    img = P.input_image()
    pt = plain_pt()
    write_result(pt, img)
    assert set_pres(pt, pw, ph) == 0
    want = R.no_tonemap_display(R.host_sum(exe, d, img, pw, ph))
    for tm in (OFF, T.TonemapSettings()):
        pt._check(c_present(pt, tm, RGBA32F)); b32, g32 = device_display(pt, RGBA32F, pw, ph); b32 = b32.copy()
        pt._check(c_present(pt, tm, RGBA8)); b8, g8 = device_display(pt, RGBA8, pw, ph)
        assert same(b8, P.quantise(b32)) and (g32 == 0xA5).all() and (g8 == 0xA5).all() and len(g8) == GUARD
        if tm is OFF:
            assert same(b32, want)
        else:
            assert P.err(b32, R.present_scaled(img, pw, ph, P.DEFAULTS, dtype=np.float64)) < 1e-3
    pt.Dispose()


def test_equal_sizes_run_todays_kernels():
    """5. SetPresentationSize(W, H), and (0, 0) after a scaled present and bloom, give the output of a context that never heard of a presentation size, bit for bit."""
    img = P.input_image(); bimg = B.input_image((W, H, 1.5, 3.8, 3))
    tm, bs = T.TonemapSettings(), T.BloomSettings()
    plain = plain_pt(); write_result(plain, img)
    want8, want32 = display(plain, tm, RGBA8, W, H), display(plain, tm, RGBA32F, W, H)
    write_result(plain, bimg); plain._check(c_bloom(plain, bs))
    want_ex, _, _ = expanded(plain, W, H); want_ex = want_ex.copy(); want_d0 = c_level(plain, 0, 0)
    assert get_pres(plain) == (W, H)
    pt = plain_pt(); write_result(pt, img)
    assert set_pres(pt, W, H) == 0 and get_pres(pt) == (W, H)
    assert same(display(pt, tm, RGBA8, W, H), want8) and same(display(pt, tm, RGBA32F, W, H), want32)
    assert set_pres(pt, 93, 53) == 0
    assert not same(display(pt, tm, RGBA8, 93, 53)[:H, :W], want8)
    write_result(pt, bimg); pt._check(c_bloom(pt, bs)); assert c_info(pt)[1:] == (46, 26)
    assert set_pres(pt, 0, 0) == 0 and get_pres(pt) == (W, H)
    buf = np.zeros((H, W, 4), np.uint8)
    assert pt._L.idkptDownloadDisplay(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION      # the buffers of the other size are gone
    pt._check(c_bloom(pt, bs))
    ex, _, _ = expanded(pt, W, H)
    assert same(ex, want_ex) and same(c_level(pt, 0, 0), want_d0) and route(pt) == T.IDKPT_BLOOM_ROUTE_TILED
    write_result(pt, img)
    assert same(display(pt, tm, RGBA8, W, H), want8) and same(display(pt, tm, RGBA32F, W, H), want32)
    plain.Dispose(); pt.Dispose()


@pytest.fixture(scope="module")
def scene(native_builder):
    return S.cornell_scene(native_builder, variant="diffuse", sky_color=(0.2, 0.3, 0.5))


CAM = S.Camera(W, H, position=(0.6, 0.4, 7.0), view_dir=(-0.08, -0.05, -1.0), fovy_deg=40.0)
CAM2 = S.Camera(W, H, position=(-0.5, 0.2, 6.0), view_dir=(0.1, -0.02, -1.0), fovy_deg=45.0)


def scene_pt(sc, **kw):
    from idkengine_amd.pathtracer import PathTracer
    pt = PathTracer(W, H, **kw)
    pt.UploadScene(sc); pt.SetCamera(CAM); pt.RayDepth = 2
    return pt


def test_accumulation_survives_a_presentation_resize(scene):
    """6. Three samples, a presentation resize, the images and the sample count unchanged; a fourth sample gives the image of an
    uninterrupted four-sample run."""
    straight = scene_pt(scene)
    for _ in range(4):
        straight.Compute()
    want4 = straight.Result
    pt = scene_pt(scene)
    for _ in range(3):
        pt.Compute()
    before = [pt.download(i) for i in range(3)]
    assert pt.AccumulatedSamples == 3
    assert set_pres(pt, 93, 53) == 0
    assert pt.AccumulatedSamples == 3 and all(same(pt.download(i), before[i]) for i in range(3))
    shown = display(pt, T.TonemapSettings(), RGBA8, 93, 53)
    assert shown.shape == (53, 93, 4) and pt.AccumulatedSamples == 3
    assert set_pres(pt, 140, 80) == 0
    pt.Compute()
    assert pt.AccumulatedSamples == 4 and same(pt.Result, want4)
    straight.Dispose(); pt.Dispose()


def test_ring_slots_keep_their_own_buffers_and_set_size_keeps_the_presentation_size(scene, host):
    """7. Two ring slots presented at the scaled size: separate buffers, each its own frame; idkptSetSize, idkptSetFrameRing and idkptSetMaxBatch keep the presentation size."""
    exe, d = host
    pt = scene_pt(scene)
    pt.SetFrameRing(2)
    assert set_pres(pt, 93, 53) == 0
    frames = []
    for cam in (CAM, CAM2):
        slot = pt.BeginFrame(); pt.SetCamera(cam); pt.Compute(); pt.Compute()
        frames.append(slot)
    assert frames == [0, 1]
    imgs = []
    for s in frames:
        out = np.zeros((H, W, 4), np.float32)
        pt._check(pt._L.idkptDownloadFrame(pt._ctx, s, 0, out.ctypes.data, out.nbytes)); imgs.append(out)
    assert not same(imgs[0], imgs[1])
    for s in frames:
        pt._check(c_present(pt, OFF, RGBA32F, slot=s))
    p0, p1 = C.c_void_p(), C.c_void_p(); n = C.c_size_t()
    pt._check(pt._L.idkptGetDisplayDevicePtr(pt._ctx, 0, C.byref(p0), C.byref(n))); pt._check(pt._L.idkptGetDisplayDevicePtr(pt._ctx, 1, C.byref(p1), C.byref(n)))
    assert p0.value != p1.value and n.value == 53 * 93 * 16
    for s in frames:
        assert same(download(pt, RGBA32F, 93, 53, slot=s), R.no_tonemap_display(R.host_sum(exe, d, imgs[s], 93, 53)))
    pt.set_max_batch(4); assert get_pres(pt) == (93, 53)
    assert same(download(pt, RGBA32F, 93, 53, slot=1), R.no_tonemap_display(R.host_sum(exe, d, imgs[1], 93, 53)))     # (kept, like the images)
    pt.SetFrameRing(1); assert get_pres(pt) == (93, 53)
    pt.SetSize(48, 32); assert get_pres(pt) == (93, 53)
    buf = np.zeros((53, 93, 4), np.float32)
    assert pt._L.idkptDownloadDisplay(pt._ctx, -1, buf.ctypes.data, buf.nbytes) == INVALID_OPERATION                   # re-made lazily, as after every resize
    small = np.ones((32, 48, 4), np.float32); small[..., :3] = np.random.default_rng(7).uniform(0.0, 1.0, (32, 48, 3)).astype(np.float32)
    write_result(pt, small)
    assert same(display(pt, OFF, RGBA32F, 93, 53), R.no_tonemap_display(R.host_sum(exe, d, small, 93, 53)))
    assert set_pres(pt, 0, 0) == 0 and get_pres(pt) == (48, 32)
    pt.Dispose()


def test_failures():
    """8. Bad sizes; a scaled present or bloom on a row-band, single-row or strip context and on a 2-member context: INVALID_OPERATION naming idkptSetPresentationSize, nothing
    launched or allocated; equal sizes keep working there; a wrong `bytes` in idkptDownloadDisplay."""
    from idkengine_amd.pathtracer import PathTracer
    tm, bs = T.TonemapSettings(), T.BloomSettings()
    pt = plain_pt()
    for w, h in ((-1, 53), (93, -1), (0, 53), (93, 0), (-1, -1), (65537, 10)):
        assert set_pres(pt, w, h) == INVALID_ARGUMENT and "idkptSetPresentationSize" in last_error(pt) and get_pres(pt) == (W, H), (w, h)
    assert pt._L.idkptSetPresentationSize(None, 1, 1) == INVALID_ARGUMENT
    assert set_pres(pt, 93, 53) == 0
    pt._check(c_present(pt, tm, RGBA8))
    for nbytes in (H * W * 4, 53 * 93 * 4 - 4, 53 * 93 * 16):
        buf = np.zeros(53 * 93 * 16, np.uint8)
        assert pt._L.idkptDownloadDisplay(pt._ctx, -1, buf.ctypes.data, nbytes) == INVALID_ARGUMENT, nbytes
    assert set_pres(pt, 1, 1) == 0
    pt._check(c_present(pt, tm, RGBA8))                                        # a 1 x 1 display is fine; bloom needs 2 x 2
    assert c_bloom(pt, bs) == INVALID_OPERATION
    pt.Dispose()
    p = C.c_void_p(); n = C.c_size_t()
    bands = PathTracer(64, 48, row_modulo=2, row_remainder=1, row_band=8)
    rows = PathTracer(64, 48, row_modulo=3, row_remainder=0)
    strip = plain_pt(64, 48); strip.SetRowRange(8, 16)
    group = plain_pt(64, 48, devices=[0, 0])
    for what, ctx in (("bands", bands), ("rows", rows), ("strip", strip), ("group", group)):
        assert set_pres(ctx, 64, 48) == 0 and c_present(ctx, tm, RGBA8) == 0, what        # equal sizes: today's path, shards included
        assert set_pres(ctx, 96, 72) == 0 and get_pres(ctx) == (96, 72), what
        for call in (lambda: c_present(ctx, tm, RGBA8), lambda: c_present(ctx, tm, RGBA32F), lambda: c_bloom(ctx, bs)):
            assert call() == INVALID_OPERATION and "idkptSetPresentationSize" in last_error(ctx), what
        assert ctx._L.idkptGetDisplayDevicePtr(ctx._ctx, -1, C.byref(p), C.byref(n)) == INVALID_OPERATION, what      # nothing was presented, nothing allocated
        assert ctx._L.idkptGetBloomDevicePtr(ctx._ctx, -1, C.byref(p), C.byref(n)) == INVALID_OPERATION, what
        assert set_pres(ctx, 0, 0) == 0 and c_present(ctx, tm, RGBA8) == 0, what
        ctx.Dispose()


def test_python_layer(scene):
    """9. SetPresentationSize / presentation_size; Present(bloom=True) returns (ph, pw, 4) and equals the C calls; Bloom returns the expanded image of the presentation size."""
    pt = scene_pt(scene)
    pt.Compute(); pt.Compute()
    assert pt.presentation_size == (W, H)
    pt.SetPresentationSize(93, 53)
    assert pt.presentation_size == (93, 53)
    tm, bs = T.TonemapSettings(), T.BloomSettings(Threshold=0.2)
    pt._check(c_bloom(pt, bs))
    ex, _, ptr = expanded(pt, 93, 53); ex = ex.copy()
    want8 = display(pt, tm, RGBA8, 93, 53, add0=ptr)
    got8 = pt.Present(bloom=bs)
    assert got8.dtype == np.uint8 and got8.shape == (53, 93, 4) and same(got8, want8)
    got32 = pt.Present(fmt="rgba32f", bloom=bs)
    assert got32.shape == (53, 93, 4) and same(P.quantise(got32), want8)
    assert pt.Present(bloom=True).shape == (53, 93, 4) and pt.Present().shape == (53, 93, 4)
    b = pt.Bloom(bs)
    assert b.shape == (53, 93, 4) and same(b, ex) and pt.bloom_route() == T.IDKPT_BLOOM_ROUTE_TILED and pt.bloom_info()[1:] == (46, 26)
    dptr, nbytes = pt.present_device_ptr(bloom=bs)
    assert nbytes == 53 * 93 * 4 and same(read_device(pt, dptr, nbytes).reshape(53, 93, 4), want8)
    pt.SetPresentationSize(0, 0)
    assert pt.presentation_size == (W, H) and pt.Present().shape == (H, W, 4)
    with pytest.raises(Exception):
        pt.SetPresentationSize(10, 0)
    pt.Dispose()


def test_gather_display_of_a_whole_frame_rank_refuses_another_presentation_size(scene):
    """10. dist: the display rows are gathered at the render size.  Equal sizes keep working; otherwise a rank that holds the whole frame is refused by local_display (a rank
    that holds a shard by idkptPresent itself: test_failures), not by a shape assertion."""
    from idkengine_amd import dist as D
    from idkengine_amd._lib import IdkPtError
    rr = D.GpuShardRenderer(W, H, 1, 0, 0); rr.upload_scene(scene); rr.set_camera(CAM); rr.pt.RayDepth = 2
    rr.render()
    with rr.stream_ctx():
        want = rr.local_display().cpu().numpy().copy()
    rr.pt.SetPresentationSize(W, H)
    with rr.stream_ctx():
        assert same(rr.local_display().cpu().numpy(), want)
    rr.pt.SetPresentationSize(93, 53)
    with pytest.raises(IdkPtError, match="idkptSetPresentationSize"):
        rr.local_display()
    rr.pt.SetPresentationSize(0, 0)
    with rr.stream_ctx():
        assert same(rr.local_display().cpu().numpy(), want)
    rr.pt.Dispose()
