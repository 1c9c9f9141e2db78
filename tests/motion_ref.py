"""The numpy restatement of idkptCaptureMotion's motion record and of idkptReproject / idkptReprojectMoments with a lookup record, written from the contract in
include/idkpt.h ("motion-aware capture" and "temporal reprojection"), not from the C++: every operation a binary32 + - * / or floor in the header's order.  numpy's float32
array arithmetic rounds each operation correctly and fuses nothing, so the result is the contract's bit for bit; tests/test_motion_ref.py holds the host build of
csrc/motion_texel.hpp and csrc/reproject_texel.hpp to it, tests/test_gpu_motion.py the device.  The reprojection below is a text of its own (tests/reproject_ref.py is the
restatement WITHOUT a lookup record; the two must agree when the lookup record is the geometry record).

`stats` (a dict, optional) receives per-pixel masks: "history" (the pixel took history), "position" (some tap inside the image with the right id failed the position test)."""
import os
import subprocess
import numpy as np

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
FLT_MAX = np.finfo(F).max
MIN_WEIGHT = F(0.01)
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def asfloat(u):
    return np.ascontiguousarray(u, np.uint32).view(F)


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


# ---- the motion record
def prev_records(bary_x, bary_y, tri_ids, xform_ids, tris, prev_positions, prev_models):
    """(N, 4) float32: the record of N hits.  tris: (T, 4) uint32 (X, Y, Z, MeshId); prev_positions: (V, 3) float32; prev_models: (X, 3, 4) float32, row r = (R_r.x, R_r.y, R_r.z, R_r.w)"""
    bx = np.asarray(bary_x, F)[:, None]; by = np.asarray(bary_y, F)[:, None]
    t = np.asarray(tris, np.uint32).reshape(-1, 4)[np.asarray(tri_ids, np.int64)]
    P = np.asarray(prev_positions, F).reshape(-1, 3)
    R = np.asarray(prev_models, F).reshape(-1, 3, 4)[np.asarray(xform_ids, np.int64)]
    with np.errstate(all="ignore"):
        bz = (F(1.0) - bx) - by
        q0, q1, q2 = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
        l = (q0 * bx + q1 * by) + q2 * bz                                    # per component
        lx, ly, lz = l[:, 0], l[:, 1], l[:, 2]
        out = np.empty((len(l), 4), F)
        for r in range(3):
            out[:, r] = ((R[:, r, 0] * lx + R[:, r, 1] * ly) + R[:, r, 2] * lz) + R[:, r, 3]
    out[:, 3] = asfloat(np.asarray(xform_ids, np.uint32))
    return out


def motion_image(geometry, hits, tris, prev_positions, prev_models):
    """(H, W, 4) float32.  geometry: the geometry image of the same hits (a miss keeps its record); hits: W * H records with BaryX, BaryY, TriangleId, MeshTransformId, Hit"""
    g = np.asarray(geometry, F)
    out = g.reshape(-1, 4).copy()
    hit = np.asarray(hits["Hit"]).ravel() != 0
    if hit.any():
        out[hit] = prev_records(hits["BaryX"].ravel()[hit], hits["BaryY"].ravel()[hit], hits["TriangleId"].ravel()[hit], hits["MeshTransformId"].ravel()[hit], tris, prev_positions, prev_models)
    return out.reshape(g.shape)


# ---- the reprojection with a lookup record
def _d2(ax, ay, az, bx, by, bz):
    dx, dy, dz = ax - bx, ay - by, az - bz
    return (dx * dx + dy * dy) + dz * dz


def reproject(cur, n, g, lookup, hg, hc, prev_proj_view, prev_view_pos, PositionTolerance=0.02, MaxHistory=32.0, stats=None):
    """(H, W, 4) float32: the temporal image of a slot whose lookup records are `lookup` (its motion image, or g itself).  id and the miss rule come from g"""
    cur = np.asarray(cur, F); g = np.asarray(g, F); lk = np.asarray(lookup, F); hg = np.asarray(hg, F); hc = np.asarray(hc, F)
    H, W = cur.shape[:2]
    M = np.asarray(prev_proj_view, F).reshape(16); vp = np.asarray(prev_view_pos, F).reshape(3)
    n = F(n); half, one = F(0.5), F(1.0)
    none = cur.copy(); none[..., 3] = n
    with np.errstate(all="ignore"):
        tol2 = F(F(PositionTolerance) * F(PositionTolerance))
        ident = bits(g[..., 3]); miss = ident == MISS
        x, y, z = lk[..., 0], lk[..., 1], lk[..., 2]
        clip = {}
        for j in (0, 1, 3):
            c = (x * M[j] + y * M[4 + j]) + z * M[8 + j]
            clip[j] = np.where(miss, c, c + M[12 + j])
        alive = clip[3] > 0
        u = (clip[0] / clip[3] * half + half) * F(W) - half
        v = (clip[1] / clip[3] * half + half) * F(H) - half
        alive &= (u > F(-1.0)) & (u < F(W)) & (v > F(-1.0)) & (v < F(H))
        us = np.where(alive, u, F(0.0)); vs = np.where(alive, v, F(0.0))
        x0f, y0f = np.floor(us), np.floor(vs)
        fx, fy = us - x0f, vs - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        weights = ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy)
        limit = tol2 * _d2(x, y, z, vp[0], vp[1], vp[2])
        s = [np.zeros((H, W), F) for _ in range(4)]; sw = np.zeros((H, W), F)
        failed_position = np.zeros((H, W), bool)
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            ok = alive & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            tg, tc = hg[cy, cx], hc[cy, cx]
            ok_id = ok & (bits(tg[..., 3]) == ident)
            near = miss | (_d2(x, y, z, tg[..., 0], tg[..., 1], tg[..., 2]) <= limit)
            failed_position |= ok_id & ~near
            ok = ok_id & near & (np.abs(tc) <= FLT_MAX).all(axis=-1)
            for ch in range(4):
                s[ch] = np.where(ok, s[ch] + tc[..., ch] * weights[k], s[ch])
            sw = np.where(ok, sw + weights[k], sw)
        take = alive & (sw >= MIN_WEIGHT)
        h = [c / sw for c in s]
        Hc = np.fmin(h[3], F(MaxHistory)); den = Hc + n
        out = none.copy()
        for ch in range(3):
            out[..., ch] = np.where(take, (h[ch] * Hc + cur[..., ch] * n) / den, none[..., ch])
        out[..., 3] = np.where(take, den, n)
    if stats is not None:
        stats.update(history=take, position=failed_position)
    return out.astype(F)


def reproject_moments(mom, n, g, lookup, hg, hm, prev_proj_view, prev_view_pos, **kw):
    """(H, W, 4) float32: the temporal moments image (M1, M2, 0, count).  mom: the slot's moments image (m1, m2, 0, 1)"""
    cur = np.zeros_like(np.asarray(mom, F)); cur[..., :2] = np.asarray(mom, F)[..., :2]
    out = reproject(cur, n, g, lookup, hg, hm, prev_proj_view, prev_view_pos, **kw)
    out[..., 2] = F(0.0)
    return out


# ---- the host build of the kernels' per-pixel functions (tests/c_driver/motion_host.cpp)
def build_host_program(exe, sanitize=True):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *flags, "-Wall", "-Werror", os.path.join(HERE, "c_driver", "motion_host.cpp"), "-o", exe])
    return exe


def _run(exe, mode, tmp, payload):
    src, dst = os.path.join(tmp, f"{mode}_in.bin"), os.path.join(tmp, f"{mode}_out.bin")
    with open(src, "wb") as f:
        for part in payload:
            f.write(np.ascontiguousarray(part).tobytes())
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    return np.frombuffer(open(dst, "rb").read(), np.uint32)


def host_records(exe, tmp, o, d, hits, tris, prev_positions, prev_models):
    """(geometry, motion), each (N, 4) float32: what k_geom_motion_pack writes for N rays of origin o and directions d and their hits"""
    N = len(hits)
    tris = np.asarray(tris, np.uint32).reshape(-1, 4); P = np.asarray(prev_positions, F).reshape(-1, 3); R = np.asarray(prev_models, F).reshape(-1, 3, 4)
    raw = _run(exe, "record", tmp, [np.int32([N, len(tris), len(P), len(R)]), np.asarray(o, F).reshape(3), np.asarray(d, F).reshape(N, 3), np.asarray(hits["T"], F), np.asarray(hits["BaryX"], F),
                                    np.asarray(hits["BaryY"], F), np.asarray(hits["TriangleId"], np.uint32), np.asarray(hits["MeshTransformId"], np.uint32), np.asarray(hits["Hit"], np.uint32), tris, P, R]).view(F)
    return raw[:4 * N].reshape(N, 4).copy(), raw[4 * N:].reshape(N, 4).copy()


def host_texel(exe, tmp, cur, n, g, lookup, hg, hc, M, vp, PositionTolerance=0.02, MaxHistory=32.0, moments=False):
    """the extended reproject_texel (lookup: an image) or the current four-argument one (lookup = None) over a frame"""
    H, W = cur.shape[:2]
    mode = 0 if lookup is None else 1
    raw = _run(exe, "texel", tmp, [np.int32([W, H, mode, 1 if moments else 0]), F([n]), np.asarray(M, F).reshape(16), np.asarray(vp, F).reshape(3), F([PositionTolerance, MaxHistory]),
                                   np.asarray(cur, F), np.asarray(g, F), np.asarray(g if lookup is None else lookup, F), np.asarray(hg, F), np.asarray(hc, F)])
    return raw.view(F).reshape(H, W, 4)
