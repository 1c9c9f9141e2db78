"""The texture storage formats the library decodes on the device at upload (include/idkpt.h: IDKPT_TEXFMT_R8, RG8, R11G11B10F, BC4_R, BC5_RG, BC7_RGBA, BC7_SRGBA;
csrc/kernels_texture.hpp).  Two kinds of evidence, both bit for bit: idkptDownloadTexture returns the resident image the numpy expanders of tests/texfmt_ref.py (BC7: the Pillow
fixture tests/golden/texfmt) predict, and a scene with a texture in a storage format renders like the same scene with that texture expanded by the test into one of the three
resident formats — which the oracle, unchanged, renders too."""
import copy
import ctypes as C
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden")); sys.path.insert(0, HERE)
import glref_cases  # noqa: E402
import texfmt_ref as R  # noqa: E402
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
from gpu_helpers import bits, gpu_render, oracle_render, assert_equal  # noqa: E402

pytestmark = pytest.mark.gpu
CAM = lambda w, h: S.Camera(w, h, position=(0.0, 0.1, 3.0), fovy_deg=48.0)  # noqa: E731
SIZES = ((4, 4), (5, 7), (1, 1), (64, 32))          # (w, h): one block; edge blocks on both axes; the sampler's 1 x 1 shortcut; several workgroups' worth of texels


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def wall(native_builder):
    return glref_cases._sampler_scene(native_builder)


@pytest.fixture(scope="module")
def mixed(wall):
    """The sampler wall (18 non-square images, every wrap x filter) with its textures replaced round-robin by the seven storage formats: (scene for the library, the same
    scene with every image expanded into its resident format)."""
    rng = np.random.default_rng(2024)
    native, expanded = [], []
    for k, t in enumerate(wall.textures):
        n, e = R.pair(R.NEW_FORMATS[k % 7], t.data.shape[1], t.data.shape[0], rng, t.wrap_s, t.wrap_t, t.mag_filter, first=61 * k)
        native.append(n); expanded.append(e)
    a, b = copy.copy(wall), copy.copy(wall)
    a.textures, b.textures = native, expanded
    return a, b


@pytest.mark.parametrize("fmt", R.NEW_FORMATS)
def test_decode_equals_reference(fmt, wall):
    from idkengine_amd.pathtracer import PathTracer
    rng = np.random.default_rng(100 + fmt)
    sc = copy.copy(wall); sc.textures = list(wall.textures); want = []
    for k, (w, h) in enumerate(SIZES):
        data, res, img = R.random_image(fmt, w, h, rng, first=300 * k, finite=False)
        sc.textures[k] = T.TextureImage.from_storage(fmt, w, h, np.frombuffer(data, np.uint8)); want.append((res, img))
    pt = PathTracer(32, 32); pt.UploadScene(sc)
    for k, (res, img) in enumerate(want):
        got_fmt, got = pt.DownloadTexture(k)
        assert got_fmt == res == T.TEXFMT_RESIDENT[fmt] and same(got, img), (fmt, SIZES[k])
    got_fmt, got = pt.DownloadTexture(len(SIZES))                         # an image in a resident format goes straight through, as before
    assert got_fmt == T.IDKPT_TEXFMT_RGBA32F and same(got, wall.textures[len(SIZES)].data)
    pt.Dispose()


def test_bc7_every_mode_and_selector_full_and_cropped(wall):
    """All fixture blocks as one 57 x 21 block grid: at full size (228 x 84) and with width / height cropped to non-multiples of 4 over the same grid, UNORM and sRGB."""
    from idkengine_amd.pathtracer import PathTracer
    blocks, texels = R.bc7_fixture()
    assert len(blocks) <= 57 * 21
    data, full = R.bc7_pick(228, 84)
    cases = [(T.IDKPT_TEXFMT_BC7_RGBA, 228, 84), (T.IDKPT_TEXFMT_BC7_SRGBA, 228, 84), (T.IDKPT_TEXFMT_BC7_RGBA, 226, 83), (T.IDKPT_TEXFMT_BC7_SRGBA, 225, 81)]
    sc = copy.copy(wall); sc.textures = list(wall.textures)
    for k, (fmt, w, h) in enumerate(cases):
        assert (w + 3) // 4 == 57 and (h + 3) // 4 == 21
        sc.textures[k] = T.TextureImage.from_storage(fmt, w, h, np.frombuffer(data, np.uint8))
    pt = PathTracer(32, 32); pt.UploadScene(sc)
    for k, (fmt, w, h) in enumerate(cases):
        got_fmt, got = pt.DownloadTexture(k)
        assert got_fmt == T.TEXFMT_RESIDENT[fmt]
        bad = (got != full[:h, :w]).any(axis=2)
        assert got.shape == (h, w, 4) and not bad.any(), f"format {fmt} {w}x{h}: {int(bad.sum())} texels differ, first block {np.argwhere(bad)[0] // 4 if bad.any() else None}"
    pt.Dispose()


def test_mixed_formats_frames_equal_oracle(mixed, oracle_mod):
    sc, ex = mixed
    for (w, h, ov) in ((192, 112, dict(RayDepth=4, OutputAOVs=1)), (97, 61, dict(RayDepth=3, DoRaySorting=1))):
        cam = CAM(w, h)
        pt = gpu_render(sc, cam, w, h, **ov); o = oracle_render(oracle_mod, ex, cam, w, h, **ov)
        assert_equal(pt, o, aov=bool(ov.get("OutputAOVs")))
        pt.Dispose(); o.close()


def test_update_texture_across_formats(wall, oracle_mod):
    """idkptUpdateTexture: a larger BC7-sRGB image replaces RGBA32F image 3, a smaller BC5 one image 11; queued samples see the old table; then the BC7 image goes back to RGBA8."""
    from idkengine_amd.pathtracer import PathTracer
    sc = wall; w, h = 160, 96; cam = CAM(w, h)
    rng = np.random.default_rng(6)
    pt = PathTracer(w, h); pt.UploadScene(sc); pt.SetCamera(cam); pt.RayDepth = 3; pt.set_max_batch(4)
    o = oracle_mod.OraclePathTracer(sc, w, h); o.set_camera(cam); o.settings.RayDepth = 3
    for _ in range(3):                                                   # three samples queued (not yet launched) when the update arrives: they see the OLD images
        pt.Compute(); o.render()
    big, big_x = R.pair(T.IDKPT_TEXFMT_BC7_SRGBA, 13, 18, rng, T.IDKPT_WRAP_MIRRORED_REPEAT, T.IDKPT_WRAP_CLAMP_TO_EDGE, T.IDKPT_FILTER_LINEAR, first=500)
    small, small_x = R.pair(T.IDKPT_TEXFMT_BC5_RG, 3, 2, rng, T.IDKPT_WRAP_CLAMP_TO_EDGE, T.IDKPT_WRAP_REPEAT, T.IDKPT_FILTER_NEAREST)
    pt.UpdateTexture(3, big); pt.UpdateTexture(11, small)
    assert (bits(pt.Result) == bits(o.image(0))).all()                   # the three samples of the old table
    assert pt.DownloadTexture(3)[0] == T.IDKPT_TEXFMT_SRGB8_A8 and same(pt.DownloadTexture(3)[1], big_x.data) and same(pt.DownloadTexture(11)[1], small_x.data)
    o.set_texture(3, big_x); o.set_texture(11, small_x)
    pt.ResetAccumulation(); o.reset_accumulation()
    for _ in range(2):
        pt.Compute(); o.render()
    assert (bits(pt.Result) == bits(o.image(0))).all() and pt.rays().tobytes() == o.rays().tobytes() and (pt.alive_queue() == o.alive_queue()).all()
    back = T.TextureImage(rng.integers(0, 256, (5, 9, 4), dtype=np.uint8), T.IDKPT_WRAP_REPEAT, T.IDKPT_WRAP_REPEAT, T.IDKPT_FILTER_LINEAR)     # and the way back: RGBA8, straight through
    pt.UpdateTexture(3, back); o.set_texture(3, back)
    assert pt.DownloadTexture(3)[0] == T.IDKPT_TEXFMT_RGBA8 and same(pt.DownloadTexture(3)[1], back.data)
    pt.ResetAccumulation(); o.reset_accumulation()
    pt.Compute(); o.render()
    assert (bits(pt.Result) == bits(o.image(0))).all() and pt.rays().tobytes() == o.rays().tobytes() and (pt.alive_queue() == o.alive_queue()).all()
    pt.Dispose(); o.close()


def test_nonfinite_r11g11b10f_texels_defeat_the_no_emission_shortcut(wall, oracle_mod):
    """No emissive factor anywhere, base-colour images in R11G11B10F, two of them with +Inf texels: 0 x such a texel is not 0, so the last bounce's hits must be shaded
    (tex_all_finite scans the packed words: a field with exponent 31)."""
    w, h = 96, 64; cam = CAM(w, h)
    sc = copy.copy(wall)
    sc.materials = wall.materials.copy(); sc.meshes = wall.meshes.copy()
    sc.materials["EmissiveFactor"] = 0.0; sc.materials["EmissiveTexture"] = 0; sc.meshes["EmissiveBias"] = 0.0
    rng = np.random.default_rng(12)
    native, expanded = [], []
    for k, t in enumerate(wall.textures):
        tw, th = t.data.shape[1], t.data.shape[0]
        wd = np.frombuffer(R.random_image(T.IDKPT_TEXFMT_R11G11B10F, tw, th, rng)[0], "<u4").copy()
        if k == 4: wd[::3] = (wd[::3] & ~np.uint32(0x7ff)) | np.uint32(0x7c0)                       # R = +Inf in every third texel
        if k == 13: wd[1::4] = (wd[1::4] & np.uint32(0x003fffff)) | np.uint32(0x3e0 << 22)          # B = +Inf
        data = wd.astype("<u4").tobytes()
        res, img = R.expand(T.IDKPT_TEXFMT_R11G11B10F, tw, th, data)
        assert np.isinf(img).any() == (k in (4, 13)) and not np.isnan(img).any()
        native.append(T.TextureImage.from_storage(T.IDKPT_TEXFMT_R11G11B10F, tw, th, np.frombuffer(data, np.uint8), t.wrap_s, t.wrap_t, t.mag_filter))
        expanded.append(T.TextureImage(img, t.wrap_s, t.wrap_t, t.mag_filter))
    ex = copy.copy(sc); sc.textures = native; ex.textures = expanded
    pt = gpu_render(sc, cam, w, h, RayDepth=2); o = oracle_render(oracle_mod, ex, cam, w, h, RayDepth=2)
    assert same(pt.DownloadTexture(4)[1], expanded[4].data) and same(pt.DownloadTexture(13)[1], expanded[13].data)
    assert_equal(pt, o)
    pt.Dispose(); o.close()


def test_two_members_on_one_gpu(mixed, oracle_mod):
    """idkptCreate(2) on one GPU: member 1 gets the RESIDENT images and their state by device-to-device copy (dev_CloneSceneFrom)."""
    from idkengine_amd.pathtracer import PathTracer
    sc, ex = mixed; w, h = 128, 80; cam = CAM(w, h)
    o = oracle_render(oracle_mod, ex, cam, w, h, RayDepth=2)
    pt = PathTracer(w, h, devices=[0, 0]); pt.UploadScene(sc); pt.SetCamera(cam); pt.RayDepth = 2
    pt.Compute()
    assert (bits(pt.Result) == bits(o.image(0))).all()
    assert pt.DownloadTexture(5)[0] == ex.textures[5].format and same(pt.DownloadTexture(5)[1], ex.textures[5].data)
    pt.Dispose(); o.close()


def test_rejections_leave_the_context_usable(mixed, oracle_mod):
    from idkengine_amd.pathtracer import PathTracer
    sc, ex = mixed; w, h = 96, 56; cam = CAM(w, h)
    pt = PathTracer(w, h)
    fmt, tw, th = C.c_int32(), C.c_int32(), C.c_int32()
    assert pt._L.idkptDownloadTexture(pt._ctx, 0, C.byref(fmt), C.byref(tw), C.byref(th), None, 0) == 3          # no scene: INVALID_OPERATION
    pt.UploadScene(sc); pt.SetCamera(cam); pt.RayDepth = 2
    good = sc.textures[0]
    rec = T.Texture(); good.fill(rec); rec.format = 10
    assert pt._L.idkptUpdateTexture(pt._ctx, 0, C.byref(rec)) == 2                                                # format 10
    rec = T.Texture(); good.fill(rec); rec.rgba = None
    assert pt._L.idkptUpdateTexture(pt._ctx, 0, C.byref(rec)) == 2                                                # null data pointer
    bad = copy.copy(sc); bad.textures = list(sc.textures)
    bad.textures[2] = copy.copy(sc.textures[2]); bad.textures[2].format = 10
    with pytest.raises(Exception):
        pt.UploadScene(bad)                                                                                       # refused before anything of the resident scene changed
    with pytest.raises(Exception):
        pt.DownloadTexture(len(sc.textures))                                                                      # index out of range
    with pytest.raises(Exception):
        pt.DownloadTexture(-1)
    buf = np.zeros(4, np.uint8)
    assert pt._L.idkptDownloadTexture(pt._ctx, 0, C.byref(fmt), C.byref(tw), C.byref(th), buf.ctypes.data, buf.nbytes) == 2   # short buffer
    assert (fmt.value, tw.value, th.value) == (ex.textures[0].format, ex.textures[0].width, ex.textures[0].height)
    pt.Compute()
    o = oracle_render(oracle_mod, ex, cam, w, h, RayDepth=2)
    assert (bits(pt.Result) == bits(o.image(0))).all()
    pt.Dispose(); o.close()
