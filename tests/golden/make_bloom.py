"""Mints tests/golden/bloom/chain.npz: the REFERENCE's own Shaders/Bloom/compute.glsl executed by Mesa llvmpipe (oracle/glref) with the bindings and dispatches of
Source/Render/Bloom.cs:56-127, for the cases of tests/bloom_ref.py CASES on bloom_ref.input_image(case).  Works only where the read-only reference and Mesa's software
rasteriser exist (oracle.glref.glref.available()); the fixture travels.

    python tests/golden/make_bloom.py            writes the fixture
    python tests/golden/make_bloom.py --check    runs the shader again and demands the committed fixture bit for bit (exit status 1 otherwise)

The shader text is read at run time and never copied into the repository; glref.preprocess() does what the engine's preprocessor does to it, and the two `#extension`
lines preprocess() puts in front of every shader are taken out again (llvmpipe has neither extension, this shader uses none).  Nothing of the shader's own text is changed.
Textures as Bloom.SetSize makes them: two R16G16B16A16Float textures of w0 x h0 with `levels` and `levels - 1` mip levels, LINEAR_MIPMAP_NEAREST / LINEAR, clamp to
edge; the source image an RGBA32F texture (linear, clamp to edge: glref_texture2d).  oracle/glref has no call for mip levels, 16-bit formats or per-level image bindings,
so those few GL calls are made from here through the GL dispatch the shim loaded (glCreateTextures, glTextureStorage2D, glTextureParameteri, glBindImageTexture with a
level and GL_RGBA16F, glGetTextureImage with GL_HALF_FLOAT).
Per pass the shader runs twice with the same bindings and uniforms (Lod, Stage):
  1. ImgResult = an RGBA32F image of the written level's size: the value imageStore receives (`ImgResult` has no format qualifier, so the program stores into whatever
     image is bound);
  2. ImgResult = the level of the RGBA16F texture, as the reference binds it: the reference's half BITS.
Keys, per case c: down_bits_c_l / up_bits_c_l (h, w, 4) uint16 and down_f32_c_l / up_f32_c_l (h, w, 4) float32 for every level l; expand_c (H, W, 4) float32 — what the
tonemap shader's `texture(Sampler1, uv)` with uv = (pixel + 0.5) / size returns for up level 0, by a three-line compute shader of this file that does exactly that
lookup (the tonemap shader itself would tone-map the value).  `cases` holds the settings.  The inputs are not stored: bloom_ref.input_image(case) makes them."""
import ctypes as C
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import bloom_ref as R  # noqa: E402
from oracle.glref import glref as G  # noqa: E402

GL_TEXTURE_2D, GL_RGBA16F, GL_RGBA, GL_HALF_FLOAT, GL_READ_WRITE = 0x0DE1, 0x881A, 0x1908, 0x140B, 0x88BA
GL_TEXTURE_MIN_FILTER, GL_TEXTURE_MAG_FILTER, GL_TEXTURE_WRAP_S, GL_TEXTURE_WRAP_T = 0x2801, 0x2800, 0x2802, 0x2803
GL_LINEAR, GL_LINEAR_MIPMAP_NEAREST, GL_CLAMP_TO_EDGE = 0x2601, 0x2701, 0x812F
DOWNSAMPLE, UPSAMPLE = 0, 1

EXPAND_SHADER = """#version 460 core
layout(local_size_x = 8, local_size_y = 8, local_size_z = 1) in;
layout(binding = 0) restrict writeonly uniform image2D ImgResult;
layout(binding = 1) uniform sampler2D Sampler1;
void main()
{
    ivec2 imgCoord = ivec2(gl_GlobalInvocationID.xy);
    ivec2 imgSize = imageSize(ImgResult);
    if (any(greaterThanEqual(imgCoord, imgSize))) return;
    vec2 uv = (imgCoord + 0.5) / imgSize;
    imageStore(ImgResult, imgCoord, vec4(texture(Sampler1, uv).rgb, 1.0));
}
"""


def shader_source():
    src = G.preprocess("Bloom/compute.glsl", {})
    for ext in ("#extension GL_ARB_bindless_texture : require\n", "#extension GL_EXT_shader_image_load_formatted : require\n"):
        assert src.count(ext) == 1
        src = src.replace(ext, "")
    return src


class BloomShader:
    def __init__(self):
        self.L = G.gl()
        self.prog = G.compile_compute(shader_source(), "Bloom/compute.glsl")
        self.expand_prog = G.compile_compute(EXPAND_SHADER, "make_bloom.py expand")
        gpa = C.CDLL(None)._glapi_get_proc_address; gpa.restype = C.c_void_p; gpa.argtypes = [C.c_char_p]
        fn = lambda name, *args: C.CFUNCTYPE(None, *args)(gpa(name))
        self.create_textures = fn(b"glCreateTextures", C.c_uint, C.c_int, C.POINTER(C.c_uint))
        self.texture_storage = fn(b"glTextureStorage2D", C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_int)
        self.texture_parameteri = fn(b"glTextureParameteri", C.c_uint, C.c_uint, C.c_int)
        self.bind_image_level = fn(b"glBindImageTexture", C.c_uint, C.c_uint, C.c_int, C.c_ubyte, C.c_int, C.c_uint, C.c_uint)
        self.get_texture_image = fn(b"glGetTextureImage", C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_void_p)

    def half_texture(self, w, h, levels):
        """Bloom.SetSize:137-146"""
        t = C.c_uint(0)
        self.create_textures(GL_TEXTURE_2D, 1, C.byref(t))
        self.texture_parameteri(t.value, GL_TEXTURE_MIN_FILTER, GL_LINEAR_MIPMAP_NEAREST); self.texture_parameteri(t.value, GL_TEXTURE_MAG_FILTER, GL_LINEAR)
        self.texture_parameteri(t.value, GL_TEXTURE_WRAP_S, GL_CLAMP_TO_EDGE); self.texture_parameteri(t.value, GL_TEXTURE_WRAP_T, GL_CLAMP_TO_EDGE)
        self.texture_storage(t.value, levels, GL_RGBA16F, w, h)
        return t.value

    def _pass(self, tex, level, size, lod, stage):
        """One pass of Bloom.Compute into level `level` of `tex` (the samplers are bound by the caller): (RGBA16F bits, the floats imageStore received)"""
        L = self.L
        w, h = size
        L.glref_set_uniform_1i(self.prog, b"Lod", lod); L.glref_set_uniform_1i(self.prog, b"Stage", stage)
        o32 = L.glref_texture2d(w, h, None, 1, 0)
        f32 = np.full((h, w, 4), np.nan, np.float32); bits = np.zeros((h, w, 4), np.uint16)
        L.glref_bind_image(0, o32)
        L.glref_dispatch(self.prog, (w + 7) // 8, (h + 7) // 8, 1); L.glref_barrier()
        L.glref_texture_read(o32, w, h, f32.ctypes.data)
        L.glref_delete_texture(o32)
        self.bind_image_level(0, tex, level, 0, 0, GL_READ_WRITE, GL_RGBA16F)
        L.glref_dispatch(self.prog, (w + 7) // 8, (h + 7) // 8, 1); L.glref_barrier(); L.glref_finish()
        self.get_texture_image(tex, level, GL_RGBA, GL_HALF_FLOAT, bits.nbytes, bits.ctypes.data)
        return bits, f32

    def run(self, img, case):
        """Bloom.Compute(src):56-127"""
        L = self.L
        W, H, thr, maxc, minus = case
        levels, sz = R.sizes(W, H, minus)
        ubo = np.zeros(4, np.float32); ubo[0] = thr; ubo[1] = maxc            # SettingsUBO, std140: Threshold, MaxColor
        b_set = L.glref_buffer(ubo.ctypes.data, ubo.nbytes)
        img = np.ascontiguousarray(img, np.float32)
        src = L.glref_texture2d(W, H, img.ctypes.data, 1, 0)                  # PathTracer.Result: linear, clamp to edge
        if max(sz[0]) == 1:
            return self._run_single_texel(img, case, b_set, src)
        down = self.half_texture(sz[0][0], sz[0][1], levels); up = self.half_texture(sz[0][0], sz[0][1], levels - 1)
        L.glref_bind_ubo(0, b_set)
        out = {}
        # Downsampling
        L.glref_bind_texture(0, src); L.glref_bind_texture(1, 0)
        out["down", 0] = self._pass(down, 0, sz[0], 0, DOWNSAMPLE)
        L.glref_bind_texture(0, down)
        for l in range(1, levels):
            out["down", l] = self._pass(down, l, sz[l], l - 1, DOWNSAMPLE)
        # Upsampling
        l = levels - 2
        L.glref_bind_texture(1, down)
        out["up", l] = self._pass(up, l, sz[l], l + 1, UPSAMPLE)
        L.glref_bind_texture(1, up)
        for l in range(levels - 3, -1, -1):
            out["up", l] = self._pass(up, l, sz[l], l + 1, UPSAMPLE)
        ex = self._expand(W, H)
        err = L.glref_error()
        L.glref_bind_texture(0, 0); L.glref_bind_texture(1, 0)
        for t in (src, down, up):
            L.glref_delete_texture(t)
        L.glref_delete_buffer(b_set)
        if err:
            raise RuntimeError(f"GL error 0x{err:x}")
        return out, ex

    def _run_single_texel(self, img, case, b_set, src):
        """Frames of 2 or 3 pixels a side: level 0 is 1 x 1 and `levels` is 2, but GL allots a 1 x 1 texture one mip level (glTextureStorage2D: INVALID_OPERATION), so
        Bloom.SetSize could not make its textures.  The shader still runs pass for pass when each level of the down chain is a one-level 1 x 1 texture of its own:
        textureLod at Lod = 1 of a one-level texture reads its only level (GL clamps the level of detail to the levels that exist), which holds what down level 1 would."""
        L = self.L
        W, H = case[0], case[1]
        down0, down1, up = self.half_texture(1, 1, 1), self.half_texture(1, 1, 1), self.half_texture(1, 1, 1)
        L.glref_bind_ubo(0, b_set)
        out = {}
        L.glref_bind_texture(0, src); L.glref_bind_texture(1, 0)
        out["down", 0] = self._pass(down0, 0, (1, 1), 0, DOWNSAMPLE)
        L.glref_bind_texture(0, down0)
        out["down", 1] = self._pass(down1, 0, (1, 1), 0, DOWNSAMPLE)
        L.glref_bind_texture(0, down1); L.glref_bind_texture(1, down1)        # level 1 of the down chain, on both units (Bloom.cs:98)
        out["up", 0] = self._pass(up, 0, (1, 1), 1, UPSAMPLE)
        L.glref_bind_texture(1, up)
        ex = self._expand(W, H)
        err = L.glref_error()
        L.glref_bind_texture(0, 0); L.glref_bind_texture(1, 0)
        for t in (src, down0, down1, up):
            L.glref_delete_texture(t)
        L.glref_delete_buffer(b_set)
        if err:
            raise RuntimeError(f"GL error 0x{err:x}")
        return out, ex

    def _expand(self, W, H):
        """what the tonemap shader reads: texture(Sampler1 = Bloom.Result, uv); unit 1 holds the up texture"""
        L = self.L
        o32 = L.glref_texture2d(W, H, None, 1, 0)
        ex = np.full((H, W, 4), np.nan, np.float32)
        L.glref_bind_image(0, o32)
        L.glref_dispatch(self.expand_prog, (W + 7) // 8, (H + 7) // 8, 1); L.glref_barrier()
        L.glref_texture_read(o32, W, H, ex.ctypes.data)
        L.glref_delete_texture(o32)
        return ex

    def close(self):
        self.L.glref_delete_program(self.prog); self.L.glref_delete_program(self.expand_prog)


def mint():
    sh = BloomShader()
    d = dict(cases=np.array(R.CASES, np.float32))
    for c, case in enumerate(R.CASES):
        out, ex = sh.run(R.input_image(case), case)
        for (chain, l), (bits, f32) in out.items():
            d[f"{chain}_bits_{c}_{l}"] = bits; d[f"{chain}_f32_{c}_{l}"] = f32
        d[f"expand_{c}"] = ex
    sh.close()
    return d


if __name__ == "__main__":
    if not G.available():
        sys.exit("make_bloom.py needs the reference's shaders and Mesa llvmpipe (oracle.glref.glref.available())")
    d = mint()
    if "--check" in sys.argv:
        fx = np.load(R.FIXTURE)
        bad = [k for k in d if k not in fx.files or fx[k].dtype != d[k].dtype or fx[k].shape != d[k].shape or fx[k].tobytes() != d[k].tobytes()] + [k for k in fx.files if k not in d]
        print("fixture reproduced bit for bit" if not bad else f"DIFFERENT: {bad}")
        sys.exit(1 if bad else 0)
    os.makedirs(os.path.dirname(R.FIXTURE), exist_ok=True)
    np.savez_compressed(R.FIXTURE, **d)
    print("wrote", R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes", {k: v.shape for k, v in d.items()})
