"""Mints tests/golden/present/agx.npz: the REFERENCE's own Shaders/TonemapAndGammaCorrect/compute.glsl executed by Mesa llvmpipe (oracle/glref) for the cases of
tests/present_ref.py CASES on present_ref.input_image().  Works only where the read-only reference and Mesa's software rasteriser exist (oracle.glref.glref.available());
the fixture travels.

    python tests/golden/make_present.py            writes the fixture
    python tests/golden/make_present.py --check    runs the shader again and demands the committed fixture bit for bit (exit status 1 otherwise)

The shader text is read at run time and never copied into the repository; glref.preprocess() does what the engine's preprocessor does to it.  Textual substitutions: the two
`#extension` lines preprocess() puts in front of every shader are taken out again (glref's A1: llvmpipe has neither extension, and this shader uses none of them).  Nothing
of the shader's own text is changed: `ImgResult` is declared without a format qualifier, so the same program stores into whatever image is bound.
Per case the shader runs twice, as TonemapAndGammaCorrect.Compute drives it: Sampler0 = an RGBA32F texture of the image's own size with the engine's filter state (linear,
clamp to edge: glref_texture2d), units 1 and 2 unbound — or unit 1 = the bloom image in the bloom case —, SettingsUBO = the six std140 words, ceil(W / 8) x ceil(H / 8) groups;
  1. ImgResult = an RGBA32F image (glref_bind_image): the value imageStore receives, before quantisation;
  2. ImgResult = an RGBA8 image, the reference's R8G8B8A8Unorm: the reference's bytes.  oracle/glref's glref_bind_image binds every image as RGBA32F, so this one binding and
     the byte read-back are two GL calls made from here (glBindImageTexture with GL_RGBA8, glGetTextureImage with GL_UNSIGNED_BYTE) through the GL dispatch the shim loaded.
The fixture holds arrays and the settings only."""
import ctypes as C
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import present_ref as R  # noqa: E402
from oracle.glref import glref as G  # noqa: E402

GL_READ_WRITE, GL_RGBA8, GL_RGBA, GL_UNSIGNED_BYTE = 0x88BA, 0x8058, 0x1908, 0x1401


def shader_source():
    src = G.preprocess("TonemapAndGammaCorrect/compute.glsl", {})
    for ext in ("#extension GL_ARB_bindless_texture : require\n", "#extension GL_EXT_shader_image_load_formatted : require\n"):
        assert src.count(ext) == 1
        src = src.replace(ext, "")
    return src


class PresentShader:
    def __init__(self):
        self.L = G.gl()
        self.prog = G.compile_compute(shader_source(), "TonemapAndGammaCorrect/compute.glsl")
        gpa = C.CDLL(None)._glapi_get_proc_address; gpa.restype = C.c_void_p; gpa.argtypes = [C.c_char_p]
        self.bind_image_fmt = C.CFUNCTYPE(None, C.c_uint, C.c_uint, C.c_int, C.c_ubyte, C.c_int, C.c_uint, C.c_uint)(gpa(b"glBindImageTexture"))
        self.get_texture_image = C.CFUNCTYPE(None, C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_void_p)(gpa(b"glGetTextureImage"))

    def run(self, img, settings, do_tonemap, bloom=None):
        L = self.L
        h, w = img.shape[:2]
        ubo = np.zeros(8, np.uint32)                                    # SettingsUBO, std140: five floats and the bool, one word each
        ubo[0:5] = np.array(settings, np.float32).view(np.uint32); ubo[5] = 1 if do_tonemap else 0
        b_set = L.glref_buffer(ubo.ctypes.data, ubo.nbytes)
        img = np.ascontiguousarray(img, np.float32)
        t0 = L.glref_texture2d(w, h, img.ctypes.data, 1, 0)             # Result: linear, clamp to edge
        t1 = 0
        if bloom is not None:
            bloom = np.ascontiguousarray(bloom, np.float32)
            t1 = L.glref_texture2d(w, h, bloom.ctypes.data, 1, 0)
        o32 = L.glref_texture2d(w, h, None, 1, 0)
        o8 = L.glref_texture2d_state(w, h, None, 1, 1, 1, 0)            # GL_RGBA8, clamp to edge, linear (TonemapAndGammaCorrect.SetSize)
        L.glref_bind_ubo(0, b_set)
        L.glref_bind_texture(0, t0); L.glref_bind_texture(1, t1); L.glref_bind_texture(2, 0)
        f32 = np.full((h, w, 4), np.nan, np.float32); u8 = np.zeros((h, w, 4), np.uint8)
        L.glref_bind_image(0, o32)
        L.glref_dispatch(self.prog, (w + 7) // 8, (h + 7) // 8, 1); L.glref_barrier()
        L.glref_texture_read(o32, w, h, f32.ctypes.data)
        self.bind_image_fmt(0, o8, 0, 0, 0, GL_READ_WRITE, GL_RGBA8)
        L.glref_dispatch(self.prog, (w + 7) // 8, (h + 7) // 8, 1); L.glref_barrier(); L.glref_finish()
        self.get_texture_image(o8, 0, GL_RGBA, GL_UNSIGNED_BYTE, u8.nbytes, u8.ctypes.data)
        err = L.glref_error()
        for t in (t0, t1, o32, o8):
            if t:
                L.glref_delete_texture(t)
        L.glref_delete_buffer(b_set)
        if err:
            raise RuntimeError(f"GL error 0x{err:x}")
        return f32, u8

    def close(self):
        self.L.glref_delete_program(self.prog)


def mint():
    sh = PresentShader()
    img, bloom = R.input_image(), R.bloom_image()
    d = dict(input=img, bloom=bloom, settings=np.array([c[:5] for c in R.CASES], np.float32), do_tonemap=np.array([c[5] for c in R.CASES], np.int32),
             with_bloom=np.array([c[6] for c in R.CASES], np.int32))
    for k, c in enumerate(R.CASES):
        d[f"float_{k}"], d[f"bytes_{k}"] = sh.run(img, c[:5], c[5], bloom if c[6] else None)
    sh.close()
    return d


if __name__ == "__main__":
    if not G.available():
        sys.exit("make_present.py needs the reference's shaders and Mesa llvmpipe (oracle.glref.glref.available())")
    d = mint()
    if "--check" in sys.argv:
        fx = np.load(R.FIXTURE)
        bad = [k for k in d if k not in fx.files or fx[k].dtype != d[k].dtype or fx[k].shape != d[k].shape or fx[k].tobytes() != d[k].tobytes()] + [k for k in fx.files if k not in d]
        print("fixture reproduced bit for bit" if not bad else f"DIFFERENT: {bad}")
        sys.exit(1 if bad else 0)
    os.makedirs(os.path.dirname(R.FIXTURE), exist_ok=True)
    np.savez_compressed(R.FIXTURE, **d)
    print("wrote", R.FIXTURE, {k: v.shape for k, v in d.items()})
