"""Mints tests/golden/adversarial_pixels/present.npz and bloom.npz: the REFERENCE's own Shaders/TonemapAndGammaCorrect/compute.glsl and Shaders/Bloom/compute.glsl executed
by Mesa llvmpipe (oracle/glref) on the images of tests/adversarial_pixels.py — every class at every size of the families present, bloom and scaled.  Works only where the
read-only reference and Mesa's software rasteriser exist (oracle.glref.glref.available()); the fixtures travel.  Outputs only: adversarial_pixels.case() makes the inputs.

    python tests/golden/make_adversarial_pixels.py            writes the fixtures
    python tests/golden/make_adversarial_pixels.py --check    runs the shaders again and demands the committed fixtures bit for bit (exit status 1 otherwise)

The shaders run through the classes of make_present_scaled.py / make_bloom.py / make_present.py (bindings and dispatches as the engine makes them; nothing of the shader's
text is changed or copied).  The one addition: Sampler2 of the tonemap shader is bound too (class overflowing_sum needs a third term).
Keys, per family f and size s ("9x5", "12x8_18x10"), arrays stacked over adversarial_pixels.CLASSES in their order:
  p_f_s_f32 / p_f_s_u8     (classes, tone settings of adversarial_pixels.TONEMAPS, 2: without / with the added images, ph, pw, 4): ImgResult as RGBA32F, and as R8G8B8A8Unorm
  b_f_s_down_l_bits / _f32, b_f_s_up_l_bits / _f32   (classes, h, w, 4): the RGBA16F bits of a level and the floats imageStore received (make_bloom.py)
  b_f_s_expand             (classes, ph, pw, 4): texture(Sampler1, uv) on up level 0
GLSL leaves min / max / clamp of a NaN undefined: what llvmpipe answers on the non-finite classes is recorded, not required (profiles/display_nonfinite.md)."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import adversarial_pixels as A  # noqa: E402
import make_present as MP  # noqa: E402
import make_present_scaled as MS  # noqa: E402
from oracle.glref import glref as G  # noqa: E402

DIR = os.path.join(HERE, "adversarial_pixels")
PRESENT_FIXTURE, BLOOM_FIXTURE = os.path.join(DIR, "present.npz"), os.path.join(DIR, "bloom.npz")


class PresentShader(MS.ScaledPresentShader):
    def run_adds(self, img, size, settings, do_tonemap, add0=None, add1=None):
        """run_scaled with Sampler2 bound as well"""
        L = self.L
        h, w = img.shape[:2]; pw, ph = size
        ubo = np.zeros(8, np.uint32)
        ubo[0:5] = np.array(settings, np.float32).view(np.uint32); ubo[5] = 1 if do_tonemap else 0
        b_set = L.glref_buffer(ubo.ctypes.data, ubo.nbytes)
        img = np.ascontiguousarray(img, np.float32)
        t0 = L.glref_texture2d(w, h, img.ctypes.data, 1, 0)
        ts = []
        for a in (add0, add1):
            if a is None:
                ts.append(0); continue
            a = np.ascontiguousarray(a, np.float32); assert a.shape == (ph, pw, 4)
            ts.append(L.glref_texture2d(pw, ph, a.ctypes.data, 1, 0))
        o32 = L.glref_texture2d(pw, ph, None, 1, 0)
        o8 = L.glref_texture2d_state(pw, ph, None, 1, 1, 1, 0)
        L.glref_bind_ubo(0, b_set)
        L.glref_bind_texture(0, t0); L.glref_bind_texture(1, ts[0]); L.glref_bind_texture(2, ts[1])
        f32 = np.full((ph, pw, 4), np.nan, np.float32); u8 = np.zeros((ph, pw, 4), np.uint8)
        L.glref_bind_image(0, o32)
        L.glref_dispatch(self.prog, (pw + 7) // 8, (ph + 7) // 8, 1); L.glref_barrier()
        L.glref_texture_read(o32, pw, ph, f32.ctypes.data)
        self.bind_image_fmt(0, o8, 0, 0, 0, MP.GL_READ_WRITE, MP.GL_RGBA8)
        L.glref_dispatch(self.prog, (pw + 7) // 8, (ph + 7) // 8, 1); L.glref_barrier(); L.glref_finish()
        self.get_texture_image(o8, 0, MP.GL_RGBA, MP.GL_UNSIGNED_BYTE, u8.nbytes, u8.ctypes.data)
        err = L.glref_error()
        L.glref_bind_texture(1, 0); L.glref_bind_texture(2, 0)
        for t in (t0, ts[0], ts[1], o32, o8):
            if t:
                L.glref_delete_texture(t)
        L.glref_delete_buffer(b_set)
        if err:
            raise RuntimeError(f"GL error 0x{err:x}")
        return f32, u8


def size_id(size):
    return f"{size[0]}x{size[1]}" + (f"_{size[2]}x{size[3]}" if len(size) == 4 else "")


def families(kind):
    """[(family, size)] whose display (kind "p") or bloom (kind "b") is recorded"""
    pres = [("present", s) for s in A.PRESENT_SIZES]; bloom = [("bloom", s) for s in A.BLOOM_SIZES]; scaled = [("scaled", s) for s in A.SCALED_SIZES]
    return pres + scaled if kind == "p" else bloom + scaled


def mint_present():
    sh = PresentShader()
    d = {}
    for fam, size in families("p"):
        pw, ph = (size[2], size[3]) if fam == "scaled" else size
        f = np.zeros((len(A.CLASSES), len(A.TONEMAPS), 2, ph, pw, 4), np.float32); u = np.zeros(f.shape, np.uint8)
        for i, cls in enumerate(A.CLASSES):
            c = A.case(fam, size, cls)
            for t, tm in enumerate(A.TONEMAPS):
                for a in (0, 1):
                    f[i, t, a], u[i, t, a] = sh.run_adds(c.img, (pw, ph), tm[:5], tm[5], c.add0 if a else None, c.add1 if a else None)
        d[f"p_{fam}_{size_id(size)}_f32"] = f; d[f"p_{fam}_{size_id(size)}_u8"] = u
    sh.close()
    return d


def mint_bloom():
    sh = MS.ScaledBloomShader()
    d = {}
    for fam, size in families("b"):
        per = {}
        for cls in A.CLASSES:
            c = A.case(fam, size, cls)
            out, ex = sh.run_scaled(c.img, A.bloom_case(c))
            for (chain, l), (bits, f32) in out.items():
                per.setdefault(f"{chain}_{l}_bits", []).append(bits); per.setdefault(f"{chain}_{l}_f32", []).append(f32)
            per.setdefault("expand", []).append(ex)
        for k, v in per.items():
            d[f"b_{fam}_{size_id(size)}_{k}"] = np.stack(v)
    sh.close()
    return d


if __name__ == "__main__":
    if not G.available():
        sys.exit("make_adversarial_pixels.py needs the reference's shaders and Mesa llvmpipe (oracle.glref.glref.available())")
    made = ((mint_present(), PRESENT_FIXTURE), (mint_bloom(), BLOOM_FIXTURE))
    if "--check" in sys.argv:
        bad = [k for d, path in made for k in MS.differences(d, path)]
        print("fixtures reproduced bit for bit" if not bad else f"DIFFERENT: {bad}")
        sys.exit(1 if bad else 0)
    for d, path in made:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, **d)
        print("wrote", path, os.path.getsize(path), "bytes", len(d), "arrays")
