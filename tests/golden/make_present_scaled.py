"""Mints tests/golden/present_scaled/cases.npz and bloom.npz: the REFERENCE's own Shaders/TonemapAndGammaCorrect/compute.glsl and Shaders/Bloom/compute.glsl executed by
Mesa llvmpipe (oracle/glref) the way Application.SetResolutions(renderRes, presentRes) (Source/Application.cs:570-586) sizes them: Sampler0 / the bloom source at the RENDER
size, ImgResult, Sampler1 and the bloom chain at the PRESENTATION size.  Works only where the read-only reference and Mesa's software rasteriser exist
(oracle.glref.glref.available()); the fixtures travel.

    python tests/golden/make_present_scaled.py            writes the fixtures
    python tests/golden/make_present_scaled.py --check    runs the shaders again and demands the committed fixtures bit for bit (exit status 1 otherwise)

The shader text is read at run time and never copied (make_present.py / make_bloom.py shader_source()); the GL plumbing is theirs too (PresentShader, BloomShader): the
classes below only separate the size of the source texture from the size of what is written.
cases.npz  per entry of present_scaled_ref.entries() (six ImgResult sizes of the 70 x 40 input, 9 x 7 of a 3 x 2 input; present_ref.CASES 0, 1 and 9): float_<key> the
           RGBA32F ImgResult (the value imageStore receives), bytes_<key> the R8G8B8A8Unorm ImgResult.  700 x 400 is held for case 0 only, and only its rows
           present_scaled_ref.BIG_ROWS (every 13th: all phases of the dither), so that the file stays below the 1 MiB a committed file may have (the whole entry's floats alone are 4.5 MB before compression).
bloom.npz  per chain c of present_scaled_ref.BLOOM_CHAINS: down_bits_c_l / up_bits_c_l / down_f32_c_l / up_f32_c_l per level and expand_c, as make_bloom.py names them.
The fixtures hold arrays only; the inputs are made by formula (present_ref.input_image, present_scaled_ref.small_image / bloom_image / bloom_source)."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import bloom_ref as B  # noqa: E402
import present_ref as P  # noqa: E402
import present_scaled_ref as R  # noqa: E402
import make_bloom as MB  # noqa: E402
import make_present as MP  # noqa: E402
from oracle.glref import glref as G  # noqa: E402


class ScaledPresentShader(MP.PresentShader):
    def run_scaled(self, img, size, settings, do_tonemap, bloom=None):
        """TonemapAndGammaCorrect.Compute with Sampler0 = img (its own size) and ImgResult (and Sampler1 = bloom) of `size` = (pw, ph)"""
        L = self.L
        h, w = img.shape[:2]; pw, ph = size
        ubo = np.zeros(8, np.uint32)
        ubo[0:5] = np.array(settings, np.float32).view(np.uint32); ubo[5] = 1 if do_tonemap else 0
        b_set = L.glref_buffer(ubo.ctypes.data, ubo.nbytes)
        img = np.ascontiguousarray(img, np.float32)
        t0 = L.glref_texture2d(w, h, img.ctypes.data, 1, 0)             # Result at the render size: linear, clamp to edge
        t1 = 0
        if bloom is not None:
            bloom = np.ascontiguousarray(bloom, np.float32); assert bloom.shape == (ph, pw, 4)
            t1 = L.glref_texture2d(pw, ph, bloom.ctypes.data, 1, 0)
        o32 = L.glref_texture2d(pw, ph, None, 1, 0)
        o8 = L.glref_texture2d_state(pw, ph, None, 1, 1, 1, 0)
        L.glref_bind_ubo(0, b_set)
        L.glref_bind_texture(0, t0); L.glref_bind_texture(1, t1); L.glref_bind_texture(2, 0)
        f32 = np.full((ph, pw, 4), np.nan, np.float32); u8 = np.zeros((ph, pw, 4), np.uint8)
        L.glref_bind_image(0, o32)
        L.glref_dispatch(self.prog, (pw + 7) // 8, (ph + 7) // 8, 1); L.glref_barrier()
        L.glref_texture_read(o32, pw, ph, f32.ctypes.data)
        self.bind_image_fmt(0, o8, 0, 0, 0, MP.GL_READ_WRITE, MP.GL_RGBA8)
        L.glref_dispatch(self.prog, (pw + 7) // 8, (ph + 7) // 8, 1); L.glref_barrier(); L.glref_finish()
        self.get_texture_image(o8, 0, MP.GL_RGBA, MP.GL_UNSIGNED_BYTE, u8.nbytes, u8.ctypes.data)
        err = L.glref_error()
        for t in (t0, t1, o32, o8):
            if t:
                L.glref_delete_texture(t)
        L.glref_delete_buffer(b_set)
        if err:
            raise RuntimeError(f"GL error 0x{err:x}")
        return f32, u8


class ScaledBloomShader(MB.BloomShader):
    def run_scaled(self, img, case):
        """Bloom.Compute(src) with the chain sized from case = (pw, ph, ...) and src = img at its own size"""
        L = self.L
        pw, ph, thr, maxc, minus = case
        H, W = img.shape[:2]
        levels, sz = B.sizes(pw, ph, minus)
        ubo = np.zeros(4, np.float32); ubo[0] = thr; ubo[1] = maxc
        b_set = L.glref_buffer(ubo.ctypes.data, ubo.nbytes)
        img = np.ascontiguousarray(img, np.float32)
        src = L.glref_texture2d(W, H, img.ctypes.data, 1, 0)
        if max(sz[0]) == 1:
            return self._run_single_texel(img, case, b_set, src)     # (reads case[0:2] for the expanded size only)
        down = self.half_texture(sz[0][0], sz[0][1], levels); up = self.half_texture(sz[0][0], sz[0][1], levels - 1)
        L.glref_bind_ubo(0, b_set)
        out = {}
        L.glref_bind_texture(0, src); L.glref_bind_texture(1, 0)
        out["down", 0] = self._pass(down, 0, sz[0], 0, MB.DOWNSAMPLE)
        L.glref_bind_texture(0, down)
        for l in range(1, levels):
            out["down", l] = self._pass(down, l, sz[l], l - 1, MB.DOWNSAMPLE)
        l = levels - 2
        L.glref_bind_texture(1, down)
        out["up", l] = self._pass(up, l, sz[l], l + 1, MB.UPSAMPLE)
        L.glref_bind_texture(1, up)
        for l in range(levels - 3, -1, -1):
            out["up", l] = self._pass(up, l, sz[l], l + 1, MB.UPSAMPLE)
        ex = self._expand(pw, ph)
        err = L.glref_error()
        L.glref_bind_texture(0, 0); L.glref_bind_texture(1, 0)
        for t in (src, down, up):
            L.glref_delete_texture(t)
        L.glref_delete_buffer(b_set)
        if err:
            raise RuntimeError(f"GL error 0x{err:x}")
        return out, ex


def mint_present():
    sh = ScaledPresentShader()
    d = {}
    for key, img, (pw, ph), c in R.entries():
        case = P.CASES[c]
        f32, u8 = sh.run_scaled(img, (pw, ph), case[:5], case[5], R.case_add(c, pw, ph))
        assert (f32[..., 3] == 1.0).all() and np.isfinite(f32).all()
        d["float_" + key] = f32[R.BIG_ROWS] if (pw, ph) == R.BIG else f32
        d["bytes_" + key] = u8[R.BIG_ROWS] if (pw, ph) == R.BIG else u8
    sh.close()
    return d


def mint_bloom():
    sh = ScaledBloomShader()
    d = dict(chains=np.array(R.BLOOM_CHAINS, np.int32), settings=np.array(R.BLOOM_SETTINGS, np.float32))
    for c, (W, H, pw, ph) in enumerate(R.BLOOM_CHAINS):
        out, ex = sh.run_scaled(R.bloom_source(W, H), (pw, ph) + R.BLOOM_SETTINGS)
        for (chain, l), (bits, f32) in out.items():
            d[f"{chain}_bits_{c}_{l}"] = bits; d[f"{chain}_f32_{c}_{l}"] = f32
        d[f"expand_{c}"] = ex
    sh.close()
    return d


def differences(d, path):
    fx = np.load(path)
    return [k for k in d if k not in fx.files or fx[k].dtype != d[k].dtype or fx[k].shape != d[k].shape or fx[k].tobytes() != d[k].tobytes()] + [k for k in fx.files if k not in d]


if __name__ == "__main__":
    if not G.available():
        sys.exit("make_present_scaled.py needs the reference's shaders and Mesa llvmpipe (oracle.glref.glref.available())")
    made = ((mint_present(), R.FIXTURE), (mint_bloom(), R.BLOOM_FIXTURE))
    if "--check" in sys.argv:
        bad = [k for d, path in made for k in differences(d, path)]
        print("fixtures reproduced bit for bit" if not bad else f"DIFFERENT: {bad}")
        sys.exit(1 if bad else 0)
    for d, path in made:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, **d)
        print("wrote", path, os.path.getsize(path), "bytes", len(d), "arrays")
