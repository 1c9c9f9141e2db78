"""Mints tests/golden/sky/atmosphere.npz: the REFERENCE's own Shaders/AtmosphericScattering/compute.glsl executed by Mesa llvmpipe (oracle/glref) for the cases of
tests/sky_ref.py CASES.  Works only where the read-only reference and Mesa's software rasteriser exist (oracle.glref.glref.available()); the fixture travels.

    python tests/golden/make_sky.py            writes the fixture
    python tests/golden/make_sky.py --check    runs the shader again and demands the committed fixture bit for bit (exit status 1 otherwise)

The shader text is read at run time and never copied into the repository; glref.preprocess() does what the engine's preprocessor does to it.  oracle/glref's shim binds
images non-layered and reads back one face, so three textual replacements — ours, in the manner of glref.py's A1-A9, none touching the arithmetic — route the result through
a storage buffer instead of the cube image:
 S1  `layout(binding = 0) restrict writeonly uniform imageCube ImgResult;` -> an SSBO of vec4 (binding 0) + `uniform int GlrefSkySize;`
 S2  `imageSize(ImgResult)` -> `ivec2(GlrefSkySize)`
 S3  `imageStore(ImgResult, imgCoord, vec4(color, 1.0));` -> a store to Texel[(face * S + y) * S + x], guarded by x < S && y < S (GL discards image stores outside the image:
     the invocations of edge workgroups beyond the face write nothing)
The fixture holds arrays and the settings only."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))
import sky_ref  # noqa: E402
from oracle.glref import glref as G  # noqa: E402

_DECL = "layout(binding = 0) restrict writeonly uniform imageCube ImgResult;"
_STORE = "imageStore(ImgResult, imgCoord, vec4(color, 1.0));"


def shader_source():
    src = G.preprocess("AtmosphericScattering/compute.glsl", {})
    src = src.replace("#extension GL_ARB_bindless_texture : require\n", "")                                    # glref A1: llvmpipe has no bindless textures (the shader uses none)
    src = src.replace("#extension GL_EXT_shader_image_load_formatted : require\n", "")                        # (no image is left to load from)
    for old, new in ((_DECL, "layout(std430, binding = 0) restrict writeonly buffer GlrefSkySSBO { vec4 Texel[]; } glrefSkySSBO;\nuniform int GlrefSkySize;"),                 # S1
                     ("imageSize(ImgResult)", "ivec2(GlrefSkySize)"),                                                                                                      # S2
                     (_STORE, "if (imgCoord.x < GlrefSkySize && imgCoord.y < GlrefSkySize) glrefSkySSBO.Texel[(imgCoord.z * GlrefSkySize + imgCoord.y) * GlrefSkySize + imgCoord.x] = vec4(color, 1.0);")):   # S3
        assert src.count(old) == 1, f"the reference's shader no longer contains exactly one `{old}`"
        src = src.replace(old, new)
    return src


class SkyShader:
    def __init__(self):
        self.L = G.gl()
        self.prog = G.compile_compute(shader_source(), "AtmosphericScattering/compute.glsl")

    def run(self, S, isteps, jsteps, light, azimuth, elevation):
        L = self.L
        ubo = np.zeros(8, np.uint32)                                    # SettingsUBO, std140: int int float float float
        ubo[0], ubo[1] = isteps, jsteps
        ubo[2:5] = np.array([max(np.float32(light), np.float32(0.0)), azimuth, elevation], np.float32).view(np.uint32)   # AtmosphericScatterer.Compute clamps LightIntensity
        out = np.full((6, S, S, 4), np.nan, np.float32)
        b_set = L.glref_buffer(ubo.ctypes.data, ubo.nbytes); b_out = L.glref_buffer(out.ctypes.data, out.nbytes)
        L.glref_bind_ubo(0, b_set); L.glref_bind_ssbo(0, b_out)
        L.glref_set_uniform_1i(self.prog, b"GlrefSkySize", S)
        L.glref_dispatch(self.prog, (S + 7) // 8, (S + 7) // 8, 6); L.glref_barrier()
        L.glref_buffer_read(b_out, 0, out.nbytes, out.ctypes.data)
        err = L.glref_error()
        L.glref_delete_buffer(b_set); L.glref_delete_buffer(b_out)
        if err:
            raise RuntimeError(f"GL error 0x{err:x}")
        return out

    def close(self):
        self.L.glref_delete_program(self.prog)


def mint():
    sh = SkyShader()
    faces = [sh.run(*c) for c in sky_ref.CASES]
    sh.close()
    c = np.array(sky_ref.CASES, np.float64)
    d = dict(sizes=c[:, 0].astype(np.int32), isteps=c[:, 1].astype(np.int32), jsteps=c[:, 2].astype(np.int32),
             light=c[:, 3].astype(np.float32), azimuth=c[:, 4].astype(np.float32), elevation=c[:, 5].astype(np.float32))
    for k, f in enumerate(faces):
        d[f"faces_{k}"] = f
    return d


if __name__ == "__main__":
    if not G.available():
        sys.exit("make_sky.py needs the reference's shaders and Mesa llvmpipe (oracle.glref.glref.available())")
    d = mint()
    if "--check" in sys.argv:
        fx = np.load(sky_ref.FIXTURE)
        bad = [k for k in d if k not in fx.files or fx[k].dtype != d[k].dtype or fx[k].shape != d[k].shape or fx[k].tobytes() != d[k].tobytes()] + [k for k in fx.files if k not in d]
        print("fixture reproduced bit for bit" if not bad else f"DIFFERENT: {bad}")
        sys.exit(1 if bad else 0)
    os.makedirs(os.path.dirname(sky_ref.FIXTURE), exist_ok=True)
    np.savez_compressed(sky_ref.FIXTURE, **d)
    print("wrote", sky_ref.FIXTURE, {k: v.shape for k, v in d.items()})
