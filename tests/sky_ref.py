"""Reference of the sky the library produces on the device (idkptComputeSky / idkptUpdateSky; csrc/kernels_sky.hpp), written in numpy from the arithmetic of
Shaders/AtmosphericScattering/compute.glsl (glsl-atmosphere adapted to a cube map) and include/Math.glsl:17-39, 139-153, independently of the kernel.

atmosphere(S, settings, dtype) evaluates the six S x S faces:
  dtype = np.float32   the shader's operation sequence, operation for operation, every intermediate rounded to binary32 (what the kernel restates);
  dtype = np.float64   "the formula's value": the same formula in binary64 with the constants as the shader writes them — the yardstick both binary32 executions
                       (the reference's shader on llvmpipe, tests/golden/sky/atmosphere.npz; this restatement; the device) are measured against.
err(X, T) is the error measure of the issue: max |X - T| / (|T| + 1e-3 max T) over R, G, B.
unorm8_to_float / srgb8_to_float are the 8-bit expansions idkptUpdateSky must reproduce (GL 4.6 8.24: UNORM c / 255 in binary32; sRGB the specification's transfer function on
R, G, B — evaluated in binary64 per byte value and rounded once, the table include/idkpt.h documents for IDKPT_TEXFMT_SRGB8_A8 — alpha linear)."""
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sky", "atmosphere.npz")

# (S, ISteps, JSteps, LightIntensity, Azimuth, Elevation): the fixture's cases
CASES = (
    (8, 40, 8, 15.0, 0.0, 0.0),       # the reference's defaults (AtmosphericScatterer.GpuSettings)
    (5, 40, 8, 15.0, 2.0, 1.45),      # a low sun; S is no multiple of the shader's workgroup nor of any grid
    (8, 1, 1, 15.0, 0.0, 0.0),        # one step of each loop
    (4, 40, 8, 0.0, 0.0, 0.0),        # no light: exactly zero, alpha 1
    (8, 16, 4, 15.0, 0.0, 3.0),       # the sun below the horizon: most of the sky near zero
)
LOW_SUN = CASES[1]


def directions(S, dtype):
    """GetWorldSpaceDirection(ndc, face) for every texel: (6, S, S, 3); ndc = (xy + 0.5) / S * 2 - 1."""
    f = dtype
    c = (np.arange(S, dtype=f) + f(0.5)) / f(S) * f(2.0) - f(1.0)
    x = np.broadcast_to(c[None, :], (S, S)); y = np.broadcast_to(c[:, None], (S, S))
    one = np.ones((S, S), f)
    v = np.stack([np.stack(t, axis=-1) for t in ((one, -y, -x), (-one, -y, x), (x, one, y), (x, -one, -y), (x, -y, one), (-x, -y, -one))]).astype(f)
    return _normalize(v)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(v):
    inv = v.dtype.type(1.0) / np.sqrt(_dot(v, v))
    return v * inv[..., None]


def _rsi(r0, rd, sr):
    f = rd.dtype.type
    a = _dot(rd, rd)
    b = f(2.0) * _dot(rd, r0)
    c = _dot(r0, r0) - sr * sr
    d = b * b - f(4.0) * a * c
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(d)
        lo = (-b - sq) / (f(2.0) * a); hi = (-b + sq) / (f(2.0) * a)
    miss = d < 0
    return np.where(miss, f(1e5), lo), np.where(miss, f(-1e5), hi)


def atmosphere(S, isteps, jsteps, light, azimuth, elevation, dtype=np.float32):
    """(6, S, S, 4) array of `dtype`: the shader's main() for every texel.  light / azimuth / elevation are taken as the binary32 values the settings block holds."""
    f = dtype
    light = f(max(np.float32(light), np.float32(0.0)))                  # AtmosphericScatterer.Compute: MaxNative(LightIntensity, 0)
    az, el = f(np.float32(azimuth)), f(np.float32(elevation))
    PI = f(3.14159265)
    r = directions(S, f).reshape(-1, 3)
    sin_t = np.sin(el)
    p_sun = np.array([sin_t * np.cos(az), np.cos(el), sin_t * np.sin(az)], f) * f(1.0)
    r0 = np.array([0.0, 6376e3, 0.0], f)
    r_planet, r_atmos = f(6371e3), f(6471e3)
    k_rlh = np.array([5.5e-6, 13.0e-6, 22.4e-6], f); k_mie = f(21e-6)
    sh_rlh, sh_mie, g = f(8e3), f(1.2e3), f(0.758)

    p_sun = _normalize(p_sun)
    r = _normalize(r)
    px, py = _rsi(r0, r, r_atmos)
    out_early = px > py
    qx, _ = _rsi(r0, r, r_planet)
    py = np.minimum(py, qx)
    istep = (py - px) / f(isteps)
    n = len(r)
    i_time = np.zeros(n, f)
    total_rlh = np.zeros((n, 3), f); total_mie = np.zeros((n, 3), f)
    i_od_rlh = np.zeros(n, f); i_od_mie = np.zeros(n, f)
    mu = _dot(r, p_sun)
    mumu = mu * mu
    gg = g * g
    p_rlh = f(3.0) / (f(16.0) * PI) * (f(1.0) + mumu)
    p_mie = f(3.0) / (f(8.0) * PI) * ((f(1.0) - gg) * (mumu + f(1.0))) / (np.power(f(1.0) + gg - f(2.0) * mu * g, f(1.5)) * (f(2.0) + gg))
    with np.errstate(over="ignore", invalid="ignore"):
        for _i in range(int(isteps)):
            i_pos = r0 + r * (i_time + istep * f(0.5))[:, None]
            i_height = np.sqrt(_dot(i_pos, i_pos)) - r_planet
            od_step_rlh = np.exp(-i_height / sh_rlh) * istep
            od_step_mie = np.exp(-i_height / sh_mie) * istep
            i_od_rlh = i_od_rlh + od_step_rlh
            i_od_mie = i_od_mie + od_step_mie
            _, sy = _rsi(i_pos, p_sun, r_atmos)
            jstep = sy / f(jsteps)
            j_time = np.zeros(n, f); j_od_rlh = np.zeros(n, f); j_od_mie = np.zeros(n, f)
            for _j in range(int(jsteps)):
                j_pos = i_pos + p_sun * (j_time + jstep * f(0.5))[:, None]
                j_height = np.sqrt(_dot(j_pos, j_pos)) - r_planet
                j_od_rlh = j_od_rlh + np.exp(-j_height / sh_rlh) * jstep
                j_od_mie = j_od_mie + np.exp(-j_height / sh_mie) * jstep
                j_time = j_time + jstep
            attn = np.exp(-((k_mie * (i_od_mie + j_od_mie))[:, None] + k_rlh * (i_od_rlh + j_od_rlh)[:, None]))
            total_rlh = total_rlh + od_step_rlh[:, None] * attn
            total_mie = total_mie + od_step_mie[:, None] * attn
            i_time = i_time + istep
        color = light * (p_rlh[:, None] * k_rlh * total_rlh + (p_mie * k_mie)[:, None] * total_mie)
    color = np.where(out_early[:, None], f(0.0), color)
    assert color.dtype == np.dtype(f)
    out = np.ones((n, 4), f); out[:, :3] = color
    return out.reshape(6, S, S, 4)


def unorm8_to_float(rgba8):
    return (np.asarray(rgba8, np.uint8).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def srgb8_to_float(rgba8):
    cs = np.arange(256, dtype=np.float64) / 255.0
    lut = np.array([c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4 for c in cs], np.float64).astype(np.float32)
    a = np.asarray(rgba8, np.uint8)
    out = lut[a]
    out[..., 3] = a[..., 3].astype(np.float32) / np.float32(255.0)
    return out


def err(X, T):
    """max |X - T| / (|T| + 1e-3 max T) over R, G, B (T: the binary64 evaluation).  0 where T is identically zero and X equals it."""
    X = np.asarray(X, np.float64)[..., :3]; T = np.asarray(T, np.float64)[..., :3]
    den = np.abs(T) + 1e-3 * T.max()
    num = np.abs(X - T)
    if not np.isfinite(num).all():
        return float("inf")
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(num == 0.0, 0.0, num / den)
    return float(q.max())


def load_fixture():
    """[(case tuple, faces (6, S, S, 4) float32)] of tests/golden/sky/atmosphere.npz, in the order of CASES."""
    fx = np.load(FIXTURE)
    out = []
    for k in range(len(fx["sizes"])):
        case = (int(fx["sizes"][k]), int(fx["isteps"][k]), int(fx["jsteps"][k]), float(fx["light"][k]), float(fx["azimuth"][k]), float(fx["elevation"][k]))
        out.append((case, fx[f"faces_{k}"]))
    return out
