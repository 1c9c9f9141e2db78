"""The numpy restatement of idkptCaptureGeometry's record and of idkptReproject, written from the contract in include/idkpt.h ("temporal reprojection"), not from the
C++: every operation a binary32 + - * / or floor in the header's order.  numpy's float32 array arithmetic rounds each operation correctly and fuses nothing, so the result
is the contract's bit for bit; tests/test_reproject_ref.py holds the host build of csrc/reproject_texel.hpp to it, tests/test_gpu_reproject.py the device.

`stats` (a dict, optional) receives per-pixel masks of what decided each pixel, for the tests that must not pass vacuously: "clip_w" (!(clip.w > 0)), "offscreen" (the
previous position outside the image), "id" / "position" / "colour" (some tap inside the image rejected by that rule, in the rules' order), "history" (the pixel took
history)."""
import os
import subprocess
import numpy as np

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
FLT_MAX = np.finfo(F).max
NO_HISTORY = -2
DEFAULTS = dict(PositionTolerance=0.02, MaxHistory=32.0)                   # include/idkpt.h, profiles/reproject.md
MIN_WEIGHT = F(0.01)
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def asfloat(u):
    return np.ascontiguousarray(u, np.uint32).view(F)


# ---- the geometry image
def centre_rays(inv_proj, inv_view, W, H):
    """(o (3,), d (H, W, 3)): Math.glsl GetWorldSpaceDirection at every pixel centre, in binary32; o is the InvView translation"""
    ip = np.asarray(inv_proj, F).reshape(16); iv = np.asarray(inv_view, F).reshape(16)
    y, x = np.mgrid[0:H, 0:W]
    two, one, half = F(2.0), F(1.0), F(0.5)
    with np.errstate(all="ignore"):
        nx = (x.astype(F) + half) / F(W) * two - one
        ny = (y.astype(F) + half) / F(H) * two - one
        rx = ip[0] * nx + ip[4] * ny
        ry = ip[1] * nx + ip[5] * ny
        # mat4_mul_xyz(invView, rx, ry, -1, 0): ((m0 x + m4 y) + m8 z) + m12 w per component
        v = [((iv[k] * rx + iv[4 + k] * ry) + iv[8 + k] * F(-1.0)) + iv[12 + k] * F(0.0) for k in range(3)]
        inv = one / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        d = np.stack([v[0] * inv, v[1] * inv, v[2] * inv], -1).astype(F)
    return iv[12:15].copy(), d


def pack(o, d, T, mesh_transform_id, hit):
    """the record of every pixel: (o + d * T, asfloat(MeshTransformId)) for a hit, (d, asfloat(0xFFFFFFFF)) for a miss.  d: (..., 3); T, ids, hit: (...)"""
    o = np.asarray(o, F); d = np.asarray(d, F); T = np.asarray(T, F); hit = np.asarray(hit) != 0
    out = np.empty(d.shape[:-1] + (4,), F)
    with np.errstate(all="ignore"):
        pos = o + d * T[..., None]
    out[..., :3] = np.where(hit[..., None], pos, d)
    out[..., 3] = np.where(hit, asfloat(np.asarray(mesh_transform_id, np.uint32)), asfloat(np.full(hit.shape, MISS, np.uint32)))
    return out


# ---- the reprojection
def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def start(cur, n):
    """historySlot == IDKPT_NO_HISTORY: (cur.rgb, n)"""
    out = np.array(np.asarray(cur, F), copy=True); out[..., 3] = F(n)
    return out


def reproject(cur, n, g, hg, hc, prev_proj_view, prev_view_pos, PositionTolerance=0.02, MaxHistory=32.0, stats=None):
    """(H, W, 4) float32: the temporal image.  cur, g, hg, hc: (H, W, 4) float32; n: the slot's sample count"""
    cur = np.asarray(cur, F); g = np.asarray(g, F); hg = np.asarray(hg, F); hc = np.asarray(hc, F)
    H, W = cur.shape[:2]
    M = np.asarray(prev_proj_view, F).reshape(16); vp = np.asarray(prev_view_pos, F).reshape(3)
    n = F(n); one, half = F(1.0), F(0.5)
    with np.errstate(all="ignore"):
        tol2 = F(F(PositionTolerance) * F(PositionTolerance))
        p = g[..., :3]; px, py, pz = p[..., 0], p[..., 1], p[..., 2]
        gid = bits(g[..., 3]); miss = gid == MISS

        def clip(j):
            c = (px * M[j] + py * M[4 + j]) + pz * M[8 + j]
            return np.where(miss, c, c + M[12 + j])
        cx, cy, cw = clip(0), clip(1), clip(3)
        w_ok = cw > 0
        u = (cx / cw * half + half) * F(W) - half
        v = (cy / cw * half + half) * F(H) - half
        on = (u > F(-1.0)) & (u < F(W)) & (v > F(-1.0)) & (v < F(H))
        go = w_ok & on
        x0f = np.floor(np.where(go, u, F(0.0))); y0f = np.floor(np.where(go, v, F(0.0)))
        fx = np.where(go, u, F(0.0)) - x0f; fy = np.where(go, v, F(0.0)) - y0f
        x0 = x0f.astype(np.int64); y0 = y0f.astype(np.int64)
        wts = [(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy]
        limit = tol2 * _dist2(p, vp)
        acc = np.zeros((H, W, 4), F); accW = np.zeros((H, W), F)
        rej = {k: np.zeros((H, W), bool) for k in ("id", "position", "colour")}
        for k in range(4):
            qx = x0 + (k & 1); qy = y0 + (k >> 1)
            inside = go & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cxq = np.clip(qx, 0, W - 1); cyq = np.clip(qy, 0, H - 1)
            hgq = hg[cyq, cxq]; hcq = hc[cyq, cxq]
            id_ok = bits(hgq[..., 3]) == gid
            pos_ok = miss | (_dist2(p, hgq[..., :3]) <= limit)
            col_ok = (np.abs(hcq) <= FLT_MAX).all(axis=-1)
            rej["id"] |= inside & ~id_ok
            rej["position"] |= inside & id_ok & ~pos_ok
            rej["colour"] |= inside & id_ok & pos_ok & ~col_ok
            valid = inside & id_ok & pos_ok & col_ok
            w = wts[k]
            acc = np.where(valid[..., None], acc + hcq * w[..., None], acc)
            accW = np.where(valid, accW + w, accW)
        take = go & (accW >= MIN_WEIGHT)
        h = acc / accW[..., None]
        Hc = np.fmin(h[..., 3], F(MaxHistory))
        den = Hc + n
        blended = np.empty((H, W, 4), F)
        blended[..., :3] = (h[..., :3] * Hc[..., None] + cur[..., :3] * n) / den[..., None]
        blended[..., 3] = den
        out = np.where(take[..., None], blended, start(cur, n)).astype(F)
    if stats is not None:
        stats.update(clip_w=~w_ok, offscreen=w_ok & ~on, history=take, **rej)
    return out


# ---- the oracle's centre rays (tests/c_driver/reproject_host.cpp, mode "rays": oracle/ref_math.h GetWorldSpaceDirection)
def build_host_program(exe, sanitize=True):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, "-Wall", "-Werror", os.path.join(HERE, "c_driver", "reproject_host.cpp"), "-o", exe])
    return exe


def run_host_program(exe, mode, tmp, payload):
    src, dst = os.path.join(tmp, f"{mode}_in.bin"), os.path.join(tmp, f"{mode}_out.bin")
    with open(src, "wb") as f:
        for part in payload:
            f.write(np.ascontiguousarray(part).tobytes())
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    return np.frombuffer(open(dst, "rb").read(), np.uint32)


def host_texel(exe, tmp, cur, n, g, hg, hc, M, vp, PositionTolerance=0.02, MaxHistory=32.0):
    H, W = cur.shape[:2]
    raw = run_host_program(exe, "texel", tmp, [np.int32([W, H]), F([n]), np.asarray(M, F).reshape(16), np.asarray(vp, F).reshape(3), F([PositionTolerance, MaxHistory]),
                                                np.asarray(cur, F), np.asarray(g, F), np.asarray(hg, F), np.asarray(hc, F)])
    return raw.view(F).reshape(H, W, 4)


def host_pack(exe, tmp, o, d, T, ids, hit):
    N = len(T)
    raw = run_host_program(exe, "pack", tmp, [np.int32([N]), np.asarray(o, F), np.asarray(d, F).reshape(N, 3), np.asarray(T, F), np.asarray(ids, np.uint32), np.asarray(hit, np.uint32)])
    return raw.view(F).reshape(N, 4)


def oracle_centre_rays(exe, tmp, inv_proj, inv_view, W, H):
    raw = run_host_program(exe, "rays", tmp, [np.int32([W, H]), np.asarray(inv_proj, F).reshape(16), np.asarray(inv_view, F).reshape(16)]).view(F)
    return raw[:3].copy(), raw[3:].reshape(H, W, 3).copy()

