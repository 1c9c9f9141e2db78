"""CPU side of the texture storage formats (include/idkpt.h, IDKPT_TEXFMT_R8 .. BC7_SRGBA): the BC7 fixture covers every (mode, selector); the numpy expanders the GPU tests
compare the device decode with (tests/texfmt_ref.py) answer hand-computed cases; TextureImage.from_storage and the scene broadcast carry such images intact."""
import os
import sys
import socket
from fractions import Fraction
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import texfmt_ref as R  # noqa: E402
import make_texfmt  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_bc7_fixture_covers_every_mode_and_selector():
    blocks, texels = R.bc7_fixture()
    assert blocks.shape == (1148, 16) and texels.shape == (1148, 4, 4, 4) and blocks.dtype == np.uint8 and texels.dtype == np.uint8
    seen = {}
    for b in blocks:
        k = make_texfmt.selector_of(b); seen[k] = seen.get(k, 0) + 1
    want = {(m, s) for (m, s, _, _) in make_texfmt.pairs()}
    assert len(want) == 285
    assert {k for k in seen if k[0] < 8} == want and all(seen[k] == 4 for k in want)
    assert [m for (m, _, _, _) in make_texfmt.pairs()].count(0) == 16 and seen[(8, 0)] == 8
    reserved = blocks[:, 0] == 0
    assert reserved.sum() == 8 and (texels[reserved] == 0).all()
    modes = np.array([make_texfmt.selector_of(b)[0] for b in blocks])
    assert (texels[modes < 4][..., 3] == 255).all()                 # modes without alpha: 255


def test_r11g11b10f_known_answers():
    # 11-bit fields: 1.0 = e 15 m 0 = 0x3c0; 0.5 = 0x380; largest finite e 30 m 63 = 0x7bf = (1 + 63/64) 2^15 = 65024; smallest denormal m 1 = 2^-20; Inf 0x7c0; NaN 0x7c1
    # 10-bit field : 1.0 = 0x1e0; largest finite 0x3df = (1 + 31/32) 2^15 = 64512; smallest denormal 2^-19; Inf 0x3e0; NaN 0x3e1
    words = np.array([0x3c0 | (0x380 << 11) | (0x1e0 << 22), 0x7bf | (0x001 << 11) | (0x3df << 22), 0x7c0 | (0x7c1 << 11) | (0x001 << 22), 0x000 | (0x7ff << 11) | (0x3e0 << 22),
                      0x001 | (0x000 << 11) | (0x3e1 << 22)], "<u4")
    out = u32(R.expand_r11g11b10f(words.tobytes(), 5, 1))[0]
    one = 0x3f800000
    assert out.tolist() == [[0x3f800000, 0x3f000000, 0x3f800000, one], [0x477e0000, 0x35800000, 0x477c0000, one], [0x7f800000, 0x7fc00000, 0x36000000, one],
                            [0x00000000, 0x7fc00000, 0x7f800000, one], [0x35800000, 0x00000000, 0x7fc00000, one]]
    # every finite field value against exact rational arithmetic
    for mbits in (6, 5):
        f = np.arange(31 << mbits); got = R._ufloat(f, mbits)
        for v, g in zip(f.tolist(), got.tolist()):
            e, m = v >> mbits, v & ((1 << mbits) - 1)
            want = Fraction(m, 1 << mbits) * Fraction(1, 1 << 14) if e == 0 else (1 + Fraction(m, 1 << mbits)) * (Fraction(2) ** (e - 15))
            assert Fraction(g) == want


def _block(r0, r1, codes):
    bits = sum(c << (3 * i) for i, c in enumerate(codes))
    return bytes([r0, r1]) + bits.to_bytes(6, "little")


def test_bc4_known_answers_both_orderings():
    codes = [0, 1, 2, 3, 4, 5, 6, 7, 7, 6, 5, 4, 3, 2, 1, 0]
    # r0 > r1: n / 1785 with n = 7 r0, 7 r1, (8 - k) r0 + (k - 1) r1 — r0 = 255, r1 = 0: 1, 0, 6/7, 5/7, 4/7, 3/7, 2/7, 1/7 rounded to float32 (6/7 = 0.110110..b x 2^0: 0x3f5b6db7)
    pal7 = [0x3f800000, 0x00000000, 0x3f5b6db7, 0x3f36db6e, 0x3f124925, 0x3edb6db7, 0x3e924925, 0x3e124925]
    # r0 <= r1: n / 1275 with n = 5 r0, 5 r1, (6 - k) r0 + (k - 1) r1, 0, 1275 — r0 = 10, r1 = 200: 50, 1000, 240, 430, 620, 810 over 1275, then 0 and 1
    pal5 = [0x3d20a0a1, 0x3f48c8c9, 0x3e40c0c1, 0x3eacacad, 0x3ef8f8f9, 0x3f22a2a3, 0x00000000, 0x3f800000]
    # the same endpoints the other way round: seven-step palette
    pal7b = [0x3f48c8c9, 0x3d20a0a1, 0x3f2d88f7, 0x3f124925, 0x3eee12a5, 0x3eb79301, 0x3e81135d, 0x3e152771]
    out = u32(R.rgtc_blocks(np.frombuffer(_block(255, 0, codes) + _block(10, 200, codes) + _block(200, 10, codes) + _block(77, 77, codes), np.uint8).reshape(-1, 8))).reshape(4, 16)
    assert out[0].tolist() == [pal7[c] for c in codes] and out[1].tolist() == [pal5[c] for c in codes] and out[2].tolist() == [pal7b[c] for c in codes]
    assert out[3].view(np.float32).tolist()[:8] == [np.float32(385) / np.float32(1275)] * 6 + [0.0, 1.0]           # r0 == r1: the five-step branch
    # texel i = x + 4y, and the image layout of a 2 x 1 block grid cropped to 5 x 3
    img = R.expand_bc4(_block(255, 0, codes) + _block(10, 200, codes), 5, 3)
    assert img.shape == (3, 5, 4) and (u32(img[..., 1:]) == np.array([0, 0, 0x3f800000], np.uint32)).all()
    assert u32(img[1, :, 0]).tolist() == [pal7[4], pal7[5], pal7[6], pal7[7], pal5[4]]
    # a random sample against exact rational arithmetic rounded once (double -> float32 cannot double-round here: n / 1785 and n / 1275 are never within 2^-53 of a float32 midpoint)
    rng = np.random.default_rng(3); blocks = rng.integers(0, 256, (64, 8), dtype=np.uint8)
    got = R.rgtc_blocks(blocks)
    for b, g in zip(blocks, got.reshape(64, 16)):
        r0, r1 = int(b[0]), int(b[1]); bits = int.from_bytes(bytes(b[2:]), "little")
        for i in range(16):
            k = (bits >> (3 * i)) & 7
            if r0 > r1: want = Fraction([r0 * 7, r1 * 7][k] if k < 2 else (8 - k) * r0 + (k - 1) * r1, 1785)
            else: want = Fraction([r0 * 5, r1 * 5][k] if k < 2 else (0 if k == 6 else 1275 if k == 7 else (6 - k) * r0 + (k - 1) * r1), 1275)
            assert g[i] == np.float32(float(want))
    img5 = R.expand_bc5(_block(255, 0, codes) + _block(10, 200, codes), 4, 4)
    assert u32(img5[..., 0]).reshape(16).tolist() == [pal7[c] for c in codes] and u32(img5[..., 1]).reshape(16).tolist() == [pal5[c] for c in codes] and (img5[..., 2] == 0).all() and (img5[..., 3] == 1).all()


def test_r8_rg8_expand_and_block_layout():
    assert R.expand_r8(bytes([1, 2, 3, 4, 5, 6]), 3, 2).tolist() == [[[1, 0, 0, 255], [2, 0, 0, 255], [3, 0, 0, 255]], [[4, 0, 0, 255], [5, 0, 0, 255], [6, 0, 0, 255]]]
    assert R.expand_rg8(bytes([1, 2, 3, 4]), 1, 2).tolist() == [[[1, 2, 0, 255]], [[3, 4, 0, 255]]]
    t = np.arange(6 * 16).reshape(6, 4, 4)                         # 3 x 2 block grid: block b, texel (y, x) -> image (4 (b // 3) + y, 4 (b % 3) + x)
    img = R.blocks_to_image(t, 10, 7)
    assert img.shape == (7, 10) and img[0, 0] == 0 and img[0, 4] == 16 and img[1, 0] == 4 and img[4, 0] == 48 and img[6, 9] == 5 * 16 + 2 * 4 + 1


def test_from_storage_fills_the_record_and_checks_the_byte_count():
    want = {T.IDKPT_TEXFMT_R8: 35, T.IDKPT_TEXFMT_RG8: 70, T.IDKPT_TEXFMT_R11G11B10F: 140, T.IDKPT_TEXFMT_BC4_R: 32, T.IDKPT_TEXFMT_BC5_RG: 64, T.IDKPT_TEXFMT_BC7_RGBA: 64, T.IDKPT_TEXFMT_BC7_SRGBA: 64}
    assert [T.IDKPT_TEXFMT_R8, T.IDKPT_TEXFMT_RG8, T.IDKPT_TEXFMT_R11G11B10F, T.IDKPT_TEXFMT_BC4_R, T.IDKPT_TEXFMT_BC5_RG, T.IDKPT_TEXFMT_BC7_RGBA, T.IDKPT_TEXFMT_BC7_SRGBA] == list(range(3, 10))
    for fmt, nbytes in want.items():
        assert T.texture_storage_bytes(fmt, 5, 7) == nbytes
        data = np.arange(nbytes, dtype=np.uint8)
        t = T.TextureImage.from_storage(fmt, 5, 7, data, wrap_s=T.IDKPT_WRAP_CLAMP_TO_EDGE, wrap_t=T.IDKPT_WRAP_MIRRORED_REPEAT, mag_filter=T.IDKPT_FILTER_NEAREST)
        rec = T.Texture(); t.fill(rec)
        assert (rec.width, rec.height, rec.format, rec.wrapS, rec.wrapT, rec.magFilter) == (5, 7, fmt, 1, 2, 1) and rec.rgba == t.data.ctypes.data
        assert t.data.dtype == np.uint8 and t.data.flags.c_contiguous and t.data.tobytes() == data.tobytes()
        for wrong in (nbytes - 1, nbytes + 1):
            with pytest.raises(AssertionError):
                T.TextureImage.from_storage(fmt, 5, 7, np.zeros(wrong, np.uint8))
    with pytest.raises(AssertionError):
        T.TextureImage.from_storage(T.IDKPT_TEXFMT_RGBA8, 1, 1, np.zeros(4, np.uint8))
    old = T.TextureImage(np.zeros((3, 2, 4), np.uint8), srgb=True); rec = T.Texture(); old.fill(rec)       # the constructor is what it was
    assert (rec.width, rec.height, rec.format) == (2, 3, T.IDKPT_TEXFMT_SRGB8_A8)


def test_broadcast_scene_carries_storage_formats(monkeypatch):
    import torch.distributed as dist
    from idkengine_amd import dist as D, scenes as S
    from idkengine_amd.bvh import NativeBuilder
    rng = np.random.default_rng(8)
    bc7, _ = R.pair(T.IDKPT_TEXFMT_BC7_SRGBA, 6, 5, rng, T.IDKPT_WRAP_CLAMP_TO_EDGE, T.IDKPT_WRAP_REPEAT, T.IDKPT_FILTER_NEAREST, first=100)
    r11, _ = R.pair(T.IDKPT_TEXFMT_R11G11B10F, 3, 7, rng, T.IDKPT_WRAP_MIRRORED_REPEAT, T.IDKPT_WRAP_CLAMP_TO_EDGE, T.IDKPT_FILTER_LINEAR)
    f32 = T.TextureImage(rng.uniform(0, 1, (2, 3, 4)).astype(np.float32), 1, 2, 1); srgb = T.TextureImage(rng.integers(0, 256, (4, 2, 4), dtype=np.uint8), 2, 0, 0, srgb=True)
    sc = S.cornell_scene(NativeBuilder(), "mixed"); sc.textures = [bc7, f32, r11, srgb, rng.uniform(0, 1, (1, 1, 4)).astype(np.float32)]
    rebuilt = []
    real = D._texture_from_meta
    monkeypatch.setattr(D, "_texture_from_meta", lambda meta, raw: rebuilt.append(real(meta, raw)) or rebuilt[-1])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        out = D.broadcast_scene(sc, src=0)
    finally:
        dist.destroy_process_group()
    assert out is sc and len(rebuilt) == 5                          # what every other rank would have rebuilt from the metadata and the bytes
    for got, want in zip(rebuilt, [T.TextureImage.of(t) for t in sc.textures]):
        assert (got.format, got.width, got.height, got.wrap_s, got.wrap_t, got.mag_filter) == (want.format, want.width, want.height, want.wrap_s, want.wrap_t, want.mag_filter)
        assert got.data.dtype == want.data.dtype and got.data.shape == want.data.shape and got.data.tobytes() == want.data.tobytes()
    assert (rebuilt[0].format, rebuilt[0].width, rebuilt[0].height) == (T.IDKPT_TEXFMT_BC7_SRGBA, 6, 5) and (rebuilt[2].format, rebuilt[2].width, rebuilt[2].height) == (T.IDKPT_TEXFMT_R11G11B10F, 3, 7)


def test_fixture_is_what_the_script_mints():
    pytest.importorskip("PIL")
    blocks, texels = make_texfmt.mint()
    fb, ft = R.bc7_fixture()
    assert (blocks == fb).all() and (texels == ft).all()
