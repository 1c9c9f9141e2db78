"""Mints tests/golden/unproject/cases.npz: the REFERENCE's own Shaders/UnprojectEquirectangular/compute.glsl executed by Mesa llvmpipe (oracle/glref) with the textures,
bindings and dispatch of SkyBoxManager.LoadSkyBoxEquirectangular (Source/Render/SkyBoxManager.cs:115-146), for the cases of tests/unproject_ref.py CASES on
unproject_ref.input_image(case).  Works only where the read-only reference and Mesa's software rasteriser exist (oracle.glref.glref.available()); the fixture travels.

    python tests/golden/make_unproject.py            writes the fixture
    python tests/golden/make_unproject.py --check    runs the shader again and demands the committed fixture bit for bit (exit status 1 otherwise)

The shader text is read at run time and never copied into the repository; glref.preprocess() does what the engine's preprocessor does to it, and the two `#extension`
lines preprocess() puts in front of every shader are taken out again (llvmpipe has neither extension, this shader uses none).  Nothing of the shader's own text is changed:
oracle/glref binds images non-layered and makes RGBA32F textures only, so the few GL calls the reference makes beyond that are made from here through the GL dispatch the
shim loaded, as tests/golden/make_bloom.py does (glCreateTextures, glTextureStorage2D with GL_RGBA16F, glTextureSubImage2D with GL_RGB / GL_RGBA + GL_FLOAT,
glBindImageTexture LAYERED, glGetTextureImage with GL_HALF_FLOAT) — the cube image is stored to directly, not through a storage buffer as tests/golden/make_sky.py does.
The 2-D texture gets NO parameter: the reference configures none (GL defaults: REPEAT, NEAREST_MIPMAP_LINEAR / LINEAR, one level allocated).
Per case c the shader runs twice with the same sampler:
  1. ImgResult = an RGBA32F cube of S a side: the value imageStore receives (`ImgResult` is writeonly and has no format qualifier: the program stores into what is bound);
  2. ImgResult = the R16G16B16A16Float cube, as the reference binds it: the reference's half BITS.
Keys: pano_bits_c (H, W, 4) uint16 — the uploaded 2-D texture read back as GL_HALF_FLOAT; store_f32_c (6, S, S, 4) float32; cube_bits_c (6, S, S, 4) uint16; for cases 0
and 1 cube_dirs_c (n, 3) float32 and cube_samples_c (n, 4) float32 — texture(samplerCube, dir) on the finished cube (GL_LINEAR, seamless, as SkyBoxManager.cs:44,74
configures externalCubemapTexture) by a few-line compute shader of this file; `cases` holds CASES.  The inputs are not stored: unproject_ref.input_image(case) makes them."""
import ctypes as C
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import unproject_ref as R  # noqa: E402
from oracle.glref import glref as G  # noqa: E402

GL_TEXTURE_2D, GL_TEXTURE_CUBE_MAP, GL_RGBA16F, GL_RGBA32F, GL_RGB, GL_RGBA, GL_FLOAT, GL_HALF_FLOAT, GL_WRITE_ONLY = 0x0DE1, 0x8513, 0x881A, 0x8814, 0x1907, 0x1908, 0x1406, 0x140B, 0x88B9
GL_TEXTURE_MIN_FILTER, GL_TEXTURE_MAG_FILTER, GL_LINEAR = 0x2801, 0x2800, 0x2601
CUBE_SAMPLES = 300

SAMPLE_SHADER = """#version 460 core
layout(local_size_x = 64, local_size_y = 1, local_size_z = 1) in;
layout(binding = 1) uniform samplerCube SamplerSky;
layout(std430, binding = 0) restrict readonly buffer DirSSBO { vec4 Dir[]; } dirSSBO;
layout(std430, binding = 1) restrict writeonly buffer OutSSBO { vec4 Result[]; } outSSBO;
uniform int Count;
void main()
{
    int i = int(gl_GlobalInvocationID.x);
    if (i >= Count) return;
    outSSBO.Result[i] = texture(SamplerSky, dirSSBO.Dir[i].xyz);
}
"""


def shader_source():
    src = G.preprocess("UnprojectEquirectangular/compute.glsl", {})
    for ext in ("#extension GL_ARB_bindless_texture : require\n", "#extension GL_EXT_shader_image_load_formatted : require\n"):
        assert src.count(ext) == 1
        src = src.replace(ext, "")
    return src


class UnprojectShader:
    def __init__(self):
        self.L = G.gl()
        self.prog = G.compile_compute(shader_source(), "UnprojectEquirectangular/compute.glsl")
        self.sample_prog = G.compile_compute(SAMPLE_SHADER, "make_unproject.py cube sample")
        gpa = C.CDLL(None)._glapi_get_proc_address; gpa.restype = C.c_void_p; gpa.argtypes = [C.c_char_p]
        fn = lambda name, *args: C.CFUNCTYPE(None, *args)(gpa(name))
        self.create_textures = fn(b"glCreateTextures", C.c_uint, C.c_int, C.POINTER(C.c_uint))
        self.texture_storage = fn(b"glTextureStorage2D", C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_int)
        self.texture_sub_image = fn(b"glTextureSubImage2D", C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_void_p)
        self.texture_parameteri = fn(b"glTextureParameteri", C.c_uint, C.c_uint, C.c_int)
        self.bind_image = fn(b"glBindImageTexture", C.c_uint, C.c_uint, C.c_int, C.c_ubyte, C.c_int, C.c_uint, C.c_uint)
        self.get_texture_image = fn(b"glGetTextureImage", C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_void_p)

    def _texture(self, target, fmt, w, h):
        t = C.c_uint(0)
        self.create_textures(target, 1, C.byref(t))
        self.texture_storage(t.value, 1, fmt, w, h)
        return t.value

    def run(self, img, S, sample_dirs=None):
        L = self.L
        H, W, ch = img.shape
        img = np.ascontiguousarray(img, np.float32)
        # equirectangularTexture.Allocate(W, H, 1, R16G16B16A16Float); Upload2D(W, H, RGB | RGBA, Float, memory)
        pano = self._texture(GL_TEXTURE_2D, GL_RGBA16F, W, H)
        self.texture_sub_image(pano, 0, 0, 0, W, H, GL_RGB if ch == 3 else GL_RGBA, GL_FLOAT, img.ctypes.data)
        pano_bits = np.zeros((H, W, 4), np.uint16)
        self.get_texture_image(pano, 0, GL_RGBA, GL_HALF_FLOAT, pano_bits.nbytes, pano_bits.ctypes.data)
        L.glref_bind_texture(0, pano)
        groups = (S + 7) // 8                                               # MyMath.DivUp(Width, 8), DivUp(Height, 8), 6
        c32 = self._texture(GL_TEXTURE_CUBE_MAP, GL_RGBA32F, S, S)
        f32 = np.full((6, S, S, 4), np.nan, np.float32)
        self.bind_image(0, c32, 0, 1, 0, GL_WRITE_ONLY, GL_RGBA32F)
        L.glref_dispatch(self.prog, groups, groups, 6); L.glref_barrier(); L.glref_finish()
        self.get_texture_image(c32, 0, GL_RGBA, GL_FLOAT, f32.nbytes, f32.ctypes.data)
        # externalCubemapTexture: R16G16B16A16Float, LINEAR / LINEAR (SkyBoxManager.cs:41-45); BindImageUnit(externalCubemapTexture, 0, 0, true)
        c16 = self._texture(GL_TEXTURE_CUBE_MAP, GL_RGBA16F, S, S)
        self.texture_parameteri(c16, GL_TEXTURE_MIN_FILTER, GL_LINEAR); self.texture_parameteri(c16, GL_TEXTURE_MAG_FILTER, GL_LINEAR)
        bits = np.zeros((6, S, S, 4), np.uint16)
        self.bind_image(0, c16, 0, 1, 0, GL_WRITE_ONLY, GL_RGBA16F)
        L.glref_dispatch(self.prog, groups, groups, 6); L.glref_barrier(); L.glref_finish()
        self.get_texture_image(c16, 0, GL_RGBA, GL_HALF_FLOAT, bits.nbytes, bits.ctypes.data)
        samples = None
        if sample_dirs is not None:
            n = len(sample_dirs)
            d4 = np.zeros((n, 4), np.float32); d4[:, :3] = sample_dirs
            samples = np.full((n, 4), np.nan, np.float32)
            b_in = L.glref_buffer(d4.ctypes.data, d4.nbytes); b_out = L.glref_buffer(samples.ctypes.data, samples.nbytes)
            L.glref_bind_ssbo(0, b_in); L.glref_bind_ssbo(1, b_out); L.glref_bind_texture(1, c16)
            L.glref_set_uniform_1i(self.sample_prog, b"Count", n)
            L.glref_dispatch(self.sample_prog, (n + 63) // 64, 1, 1); L.glref_barrier()
            L.glref_buffer_read(b_out, 0, samples.nbytes, samples.ctypes.data)
            L.glref_bind_texture(1, 0)
            L.glref_delete_buffer(b_in); L.glref_delete_buffer(b_out)
        err = L.glref_error()
        L.glref_bind_texture(0, 0)
        for t in (pano, c32, c16):
            L.glref_delete_texture(t)
        if err:
            raise RuntimeError(f"GL error 0x{err:x}")
        return pano_bits, f32, bits, samples

    def close(self):
        self.L.glref_delete_program(self.prog); self.L.glref_delete_program(self.sample_prog)


def mint():
    sh = UnprojectShader()
    d = dict(cases=np.array(R.CASES, np.int32))
    for c, case in enumerate(R.CASES):
        dirs = R.cube_dirs(CUBE_SAMPLES, 99 + c) if c < 2 else None
        pano_bits, f32, bits, samples = sh.run(R.input_image(case), case[2], dirs)
        d[f"pano_bits_{c}"] = pano_bits; d[f"store_f32_{c}"] = f32; d[f"cube_bits_{c}"] = bits
        if dirs is not None:
            d[f"cube_dirs_{c}"] = dirs; d[f"cube_samples_{c}"] = samples
    sh.close()
    return d


if __name__ == "__main__":
    if not G.available():
        sys.exit("make_unproject.py needs the reference's shaders and Mesa llvmpipe (oracle.glref.glref.available())")
    d = mint()
    if "--check" in sys.argv:
        fx = np.load(R.FIXTURE)
        bad = [k for k in d if k not in fx.files or fx[k].dtype != d[k].dtype or fx[k].shape != d[k].shape or fx[k].tobytes() != d[k].tobytes()] + [k for k in fx.files if k not in d]
        print("fixture reproduced bit for bit" if not bad else f"DIFFERENT: {bad}")
        sys.exit(1 if bad else 0)
    os.makedirs(os.path.dirname(R.FIXTURE), exist_ok=True)
    np.savez_compressed(R.FIXTURE, **d)
    print("wrote", R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes", {k: v.shape for k, v in d.items()})
