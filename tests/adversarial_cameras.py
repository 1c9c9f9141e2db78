"""Adversarial cameras for the first-hit stage (numpy only, deterministic): every case puts a boundary of k_classify_tiles' decision — a silhouette, the apex of a tile's beam,
a sky-face boundary, a gate of the rule — onto or next to a tile.  tests/test_adversarial_cameras_ref.py proves on the CPU, with the oracle alone, that each case is what it
claims; tests/test_gpu_adversarial_cameras.py reads the tile classes back (idkptDownloadTileClasses) and holds them, and the frames rendered with them, to the oracle.

Scenes (idkengine_amd.scenes assembles them; closed boxes of 12 triangles on dyadic coordinates, a constant-per-face sky of six distinct colours unless a case says otherwise):
  one             one BLAS: the box [-1, 1]^2 x [-6, -4] (a case may move it)
  flat            one axis-aligned quad in the plane y = 0: the root box has zero thickness
  inst            9 instances of the unit box: identity, exact quarter turns, a mirror, a needle scale (1000, 1, 1/1000) turned 23 degrees about Y (InvModel: the binary32 inverse
                  scenes.transform_from_matrix produces), a shear
  inst256/inst257 single-triangle BLASes, at and beyond the classifier's gate of 256 instances
  same_space      4 BLASes under one InvModel (the unified tree)
  tlas_leaf_root  one instance: the TLAS root is a leaf, which UseTlas = 1 enters unconditionally — no shortcut

Truth per tile (truth()): over every pixel of the tile, the 9 x 9 jitters {0, 1/8 .. 7/8, nextafter(1, 0)}^2 and 9 lens points — the centre and 8 points on the rim of what
Sampling.glsl:98-114 SampleDisk can return: `point * 2 - 1` of a point of the unit quarter disc, so the rim reaches the corner (-1, -1), sqrt(2) lens radii off the axis —
the oracle's own primary ray (ref_primary_rays) and its own first box tests (ref_first_box_tests): can_hit = some ray passes one, faces = the sky faces those rays see.
"""
import math
import os
import sys
import ctypes as C
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

f32 = np.float32
ONE_BELOW = float(np.nextafter(f32(1.0), f32(0.0)))
JITTERS = np.float32([(a, b) for b in list(np.arange(8) / 8.0) + [ONE_BELOW] for a in list(np.arange(8) / 8.0) + [ONE_BELOW]])            # 81 (ox, oy)
_ARC = [(2.0 * math.cos(a) - 1.0, 2.0 * math.sin(a) - 1.0) for a in (math.pi / 8, math.pi / 4, 3 * math.pi / 8)]
# the centre, then the rim of SampleDisk's range: the three corners of [-1, 1)^2 it reaches, two edge midpoints, three points of the arc |p| = 1
LENS = np.float32([(0.0, 0.0), (-1.0, -1.0), (ONE_BELOW, -1.0), (-1.0, ONE_BELOW), (0.0, -1.0), (-1.0, 0.0)] + _ARC)
SKY6 = np.float32([[0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.1, 0.1, 0.9], [0.8, 0.8, 0.1], [0.1, 0.8, 0.8], [0.8, 0.1, 0.8]])
FLT_MAX = f32(3.4028235e+38)

# Cameras that once differed, by name: {"name": Case}; filled below (after Case), appended to CASES.
REGRESSION_CAMERAS = {}
LENS_RIM = 1.41422                        # k_classify_tiles: the lens reaches sqrt(2) radii off the axis (rounded up)


def ulps(x, n):
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf) if n > 0 else f32(-np.inf))
    return float(x)


# ----------------------------------------------------------------------------------------------------------------- scenes
def _box(lo, hi):
    return S._box_faces(lo, hi, with_bottom=True).reshape(-1, 3, 3)


def _mesh(tp, k=0):
    p, i, nrm, tan = S.flat_shaded(tp)
    return S.MeshInput(p, i, S.make_material((0.45 + 0.05 * (k % 8), 0.85 - 0.05 * (k % 8), 0.6, 1.0)), nrm, tan)


def _sky(sc, kind):
    if kind == "none":
        sc.sky_faces = None
    elif kind == "tex":                        # 2 x 2 texels per face, every texel its own colour
        t = np.ones((6, 2, 2, 4), np.float32)
        t[..., :3] = SKY6[:, None, None, :] * np.float32([[1.0, 0.75], [0.5, 0.25]])[None, :, :, None]
        sc.sky_faces = t
    else:
        t = np.ones((6, 1, 1, 4), np.float32); t[:, 0, 0, :3] = SKY6
        sc.sky_faces = t
    return sc


def _instanced(parts, blas_of, matrices, builder):
    sc = S.assemble([{"meshes": [_mesh(tp, k)]} for k, tp in enumerate(parts)], builder, build_tlas=False)
    inst = np.zeros(len(blas_of), T.GpuBlasInstance); inst["BlasId"] = blas_of; inst["MeshTransformId"] = np.arange(len(blas_of))
    sc.blas_instances = inst
    sc.mesh_transforms = np.concatenate([S.transform_from_matrix(m) for m in matrices])
    S.rebuild_tlas(sc, builder)
    return sc


def _quarter(axis, turns):
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][turns % 4]
    m = np.eye(4); u, v = (axis + 1) % 3, (axis + 2) % 3
    m[u, u] = c; m[u, v] = s; m[v, u] = -s; m[v, v] = c
    return m


def inst_matrices():
    Tr = S.translation
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0]); needle = np.diag([1000.0, 1.0, 1.0 / 1000.0, 1.0]); shear = np.eye(4); shear[1, 0] = 0.5; shear[2, 1] = -0.25
    return [Tr((0.0, 0.0, -5.0)), _quarter(1, 1) @ Tr((-3.0, 0.0, -6.0)), _quarter(0, 1) @ Tr((3.0, 0.0, -6.0)), _quarter(2, 2) @ Tr((0.0, 3.0, -6.0)), _quarter(1, 3) @ Tr((0.0, -3.0, -6.0)),
            mirror @ Tr((-2.0, 2.0, -7.0)), needle @ S.rotation_y(23.0) @ Tr((0.0, 0.0, -300.0)), shear @ Tr((2.5, -2.5, -7.0)), _quarter(2, 1) @ Tr((2.0, 2.0, -8.0))]


def _grid_triangles(n):
    """n single triangles on a 17-wide dyadic grid in the plane z = -8, in front of the default camera"""
    out = []
    for k in range(n):
        x, y = (k % 17 - 8) * 0.25, (k // 17 - 8) * 0.25
        out.append(np.float32([[[x, y, -8.0], [x + 0.125, y, -8.0], [x, y + 0.125, -8.0]]]))
    return out


def make_scene(name, builder, sky="faces", shift=(0.0, 0.0, 0.0), hi_x=1.0, box=None):
    if name == "one":
        lo = np.float64([-1.0, -1.0, -6.0]) + shift; hi = np.float64([hi_x, 1.0, -4.0]) + shift
        if box is not None:                    # (lo, hi) of another box
            lo, hi = np.float64(box[0]), np.float64(box[1])
        sc = S.assemble([{"meshes": [_mesh(_box(lo, hi))]}], builder)
    elif name == "flat":
        sc = S.assemble([{"meshes": [_mesh(S._quad((-1.0, 0.0, -6.0), (1.0, 0.0, -6.0), (1.0, 0.0, -4.0), (-1.0, 0.0, -4.0)))]}], builder)
    elif name == "inst":
        sc = _instanced([_box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))], [0] * 9, inst_matrices(), builder)
    elif name in ("inst256", "inst257"):
        n = int(name[4:])
        sc = _instanced(_grid_triangles(n), list(range(n)), [np.eye(4)] * n, builder)
    elif name == "same_space":
        sc = S.assemble([{"meshes": [_mesh(_box((x, y, -6.0), (x + 0.75, y + 0.75, -4.0)), k)]} for k, (x, y) in enumerate([(-1.0, -1.0), (0.25, -1.0), (-1.0, 0.25), (0.25, 0.25)])], builder)
    elif name == "tlas_leaf_root":
        sc = _instanced([_box((-1.0, -1.0, -6.0), (1.0, 1.0, -4.0))], [0], [np.eye(4)], builder)
    else:
        raise ValueError(name)
    return _sky(sc, sky)


# ----------------------------------------------------------------------------------------------------------------- cameras (raw per-frame data)
def inv_proj(fovy_deg=90.0, aspect=1.0, flip_y=False, off=(0.0, 0.0)):
    """InvProjection of a perspective projection; only [0], [1], [4], [5] reach the ray direction (Math.glsl:6-15: mat2(inverseProj) * ndc)"""
    t = math.tan(math.radians(fovy_deg) / 2.0)
    ip = np.zeros(16, np.float32)
    ip[0] = t * aspect; ip[5] = -t if flip_y else t; ip[1] = off[0]; ip[4] = off[1]; ip[11] = -1.0; ip[14] = -1.0; ip[15] = 1.0
    return ip


def inv_view(direction=(0.0, 0.0, -1.0), eye=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """InvView (OpenTK memory order: rows right, up, back, eye) looking along `direction`; an axis direction gives entries 0 and +-1 exactly"""
    d = np.float64(direction); back = -d / np.linalg.norm(d)
    up = np.float64(up) if abs(np.dot(up, back)) < 0.99 else np.float64([0.0, 0.0, 1.0])
    right = np.cross(up, back); right /= np.linalg.norm(right)
    u = np.cross(back, right)
    m = np.eye(4); m[0, :3] = right; m[1, :3] = u; m[2, :3] = back; m[3, :3] = eye
    return m.astype(np.float32)


def perframe(ip, iv, view_pos=None):
    p = np.zeros(1, T.GpuPerFrameData)
    p["InvProjection"][0] = ip; p["InvView"][0] = np.asarray(iv, np.float32).reshape(16)
    p["ViewPos"][0] = np.asarray(iv, np.float32).reshape(4, 4)[3, :3] if view_pos is None else view_pos
    return p


class Case:
    def __init__(self, name, cls, scene="one", frame=(64, 64), pf=None, focal=8.0, radius=0.0, sky="faces", expect="some", scene_kw=None, rows=None, lights=False, aovs=False, plain=True):
        self.name, self.cls, self.scene, self.frame, self.pf, self.focal, self.radius, self.sky = name, cls, scene, frame, pf, focal, radius, sky
        self.expect = expect            # "some": tiles are classified; "zero": every class must be 0; "none": the batch runs without a classification (sets == 0)
        self.scene_kw = scene_kw or {}
        self.rows = rows                # None: the whole frame; ("members", n): n members on one device; ("range", first, count): a strip
        self.lights, self.aovs = lights, aovs
        self.plain = plain              # a plain case has at least one clearly empty tile (the ref test asserts it)

    def scene_key(self):
        return (self.scene, self.sky, repr(sorted(self.scene_kw.items())))

    def settings(self, **ov):
        d = dict(RayDepth=2, FocalLength=self.focal, LenseRadius=self.radius, OutputAOVs=int(self.aovs), DoTraceLights=int(self.lights))
        d.update(ov)
        return d


def _regressions():
    # A sheared InvProjection ([4] = -[5]: the side planes of a tile have normals along (1, 1, .) / sqrt(2) in camera space) with the lens near its gate and a small box 0.6
    # from the eye: the rim of the lens — SampleDisk's corner (-1, -1), sqrt(2) radii off the axis — carried rays into the box from two tiles whose beams the rule, written
    # with the radius itself, had put beyond it by its margin.
    REGRESSION_CAMERAS["lens_sheared_near"] = Case("lens_sheared_near", "lens", pf=perframe(inv_proj(90.0, 1.0, off=(0.0, -1.0)), inv_view()), focal=8.0, radius=0.375,
                                                   scene_kw={"box": ((-0.375, -0.375, -0.5), (-0.25, -0.25, -0.375))}, plain=False)


def _default_pf(w=64, h=64, eye=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fovy=90.0, **kw):
    return perframe(inv_proj(fovy, w / float(h), **kw), inv_view(direction, eye))


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))      # noqa: E731
    px = 0.125                                           # one pixel at z = -4 under fovy 90 degrees at 64 x 64
    # silhouette_on_tile_edge: the face z = -4 of the box projects onto pixel columns / rows 24 and 40, which are tile edges
    for tag, kw in (("exact", {}), ("plus_1px", {"shift": (px, px, 0.0)}), ("minus_1px", {"shift": (-px, -px, 0.0)}), ("plus_half", {"shift": (px / 2, px / 2, 0.0)}),
                    ("minus_half", {"shift": (-px / 2, -px / 2, 0.0)}), ("plus_ulp", {"hi_x": ulps(1.0, 1)}), ("minus_ulp", {"hi_x": ulps(1.0, -1)})):
        add("silhouette_" + tag, "silhouette_on_tile_edge", pf=_default_pf(), scene_kw=kw)
    # apex: the eye inside the root box, on a face / an edge / a corner of it, the box behind the eye, the box straddling the eye's plane
    for tag, eye, expect in (("inside", (0.0, 0.0, -5.0), "zero"), ("on_face", (0.0, 0.0, -4.0), "zero"), ("on_edge", (1.0, 0.0, -4.0), "zero"), ("on_corner", (1.0, 1.0, -4.0), "zero"),
                             ("behind_on_axis", (0.0, 0.0, -8.0), "some"), ("behind_off_axis", (3.0, 0.5, -9.0), "some"), ("straddling", (2.5, 0.0, -5.0), "some")):
        add("apex_" + tag, "apex", pf=_default_pf(eye=eye), expect=expect, plain=expect == "some")
    # edge_on: the eye in the plane of the flat quad, and one ulp off it on either side (the ulp of 0 is the denormal 1.4e-45: the cases rely on denormals surviving in the oracle and in the kernels alike)
    # (off the plane the eye stands over / under the quad itself: the rays of one half of the frame meet it at once, those of the other half never)
    for tag, eye in (("in_plane", (0.0, 0.0, 0.0)), ("ulp_above", (0.0, ulps(0.0, 1), -5.0)), ("ulp_below", (0.0, ulps(0.0, -1), -5.0))):
        add("edge_on_" + tag, "edge_on", scene="flat", pf=_default_pf(eye=eye), plain=tag == "in_plane")
    # far / near
    add("far_1e4", "far", pf=_default_pf(eye=(0.03, 0.03, 1.0e4 - 5.0), fovy=90.0), plain=True)
    add("far_1e6", "far", pf=_default_pf(eye=(300.0, 300.0, 1.0e6 - 5.0)), plain=True)
    add("near_2p-10", "near", pf=_default_pf(eye=(1.0 + 2.0 ** -10, 0.0, -5.0), direction=(0.0, 0.0, -1.0)), plain=False)      # (the box reaches behind the eye's plane: no side plane of a tile has all of it beyond)
    # fov
    add("fov_1deg", "fov", pf=_default_pf(fovy=1.0, eye=(1.0, 0.0, 0.0)))                        # the box edge x = 1 down the middle of the frame
    add("fov_170deg", "fov", pf=_default_pf(fovy=170.0))
    add("fov_flip_y", "fov", pf=_default_pf(flip_y=True), scene_kw={"shift": (0.0, 1.5, 0.0)})
    add("fov_off_diagonal", "fov", pf=_default_pf(off=(0.25, -0.125)))
    # lens: LenseRadius / FocalLength at the gate 0.05 and one ulp around it, FocalLength at its gate, radius 0, the focal plane in front of / inside / behind the box
    F = 2.0
    r_gate = float(f32(0.05) * f32(F))
    while f32(r_gate) / f32(F) > f32(0.05):
        r_gate = ulps(r_gate, -1)
    while f32(ulps(r_gate, 1)) / f32(F) <= f32(0.05):
        r_gate = ulps(r_gate, 1)                         # the largest radius that still passes r / F <= 0.05f
    far = {"shift": (0.0, 0.0, -8.0)}                      # fovy 60 degrees, the box at z = -14 .. -12: the outer tiles clear the doubled margin and agree on the sky face
    lp = lambda: _default_pf(fovy=60.0)                  # noqa: E731
    add("lens_at_gate", "lens", pf=lp(), focal=F, radius=r_gate, scene_kw=far)
    add("lens_above_gate", "lens", pf=lp(), focal=F, radius=ulps(r_gate, 1), expect="zero", plain=False, scene_kw=far)
    add("lens_below_gate", "lens", pf=lp(), focal=F, radius=ulps(r_gate, -1), scene_kw=far)
    add("lens_focal_at_gate", "lens", pf=lp(), focal=float(f32(1e-3)), radius=0.0, expect="zero", plain=False, scene_kw=far)
    add("lens_focal_above_gate", "lens", pf=lp(), focal=ulps(1e-3, 1), radius=float(f32(1e-3)) * 0.04, scene_kw=far)
    add("lens_radius_0", "lens", pf=lp(), focal=F, radius=0.0, scene_kw=far)
    add("lens_focus_in_front", "lens", pf=lp(), focal=6.0, radius=0.25, scene_kw=far)
    add("lens_focus_inside", "lens", pf=lp(), focal=13.0, radius=0.25, scene_kw=far)
    add("lens_focus_behind", "lens", pf=lp(), focal=20.0, radius=0.25, scene_kw=far)
    add("lens_near_box", "lens", pf=_default_pf(eye=(1.5, 0.0, -5.0)), focal=8.0, radius=0.375, plain=False)      # the box half a unit beside the eye: the lens reaches further than the tilt
    # apex_mismatch: ViewPos a few ulps off InvView's translation
    iv = inv_view((0.0, 0.0, -1.0), (0.3, -0.2, 0.7))
    add("apex_mismatch", "apex_mismatch", pf=perframe(inv_proj(), iv, [ulps(iv[3, 0], 3), ulps(iv[3, 1], -2), ulps(iv[3, 2], 4)]), focal=4.0, radius=0.05)
    # sky_faces: view directions that put tile columns / rows on |x| = |z| (and |y|); the box far to the side so that most tiles see the sky only
    for tag, d, shift in (("x_z", (1.0, 0.0, -1.0), (5.0, 0.0, 0.0)), ("diag", (1.0, 1.0, 1.0), (5.0, 5.0, 10.0)), ("z", (0.0, 0.0, -1.0), (5.0, 0.0, 0.0))):
        add("sky_" + tag, "sky_faces", pf=_default_pf(direction=d), scene_kw={"shift": shift})
        add("sky_" + tag + "_lens", "sky_faces", pf=_default_pf(direction=d, fovy=90.0 if tag == "z" else 60.0), scene_kw={"shift": shift}, focal=F, radius=r_gate, plain=False)
    # ... and aimed at eta: the boundary |x| = |z| on pixel column 30, so the widened beam of the tiles of columns 32-39 starts one pixel (0.018 rad) inside the face +X,
    # less than the tilt of a ray from the rim of the lens (sqrt(2) * r / F = 0.07 rad): all four corners agree on the face, rays of the tile do not
    th = math.pi / 4 - math.atan(math.tan(math.radians(30.0)) * (30.0 / 32.0 - 1.0))
    add("sky_x_z_lens_aimed", "sky_faces", pf=_default_pf(direction=(math.sin(th), 0.0, -math.cos(th)), fovy=60.0), scene_kw={"shift": (5.0, 0.0, 0.0)}, focal=F, radius=r_gate, plain=False)
    add("sky_textured", "sky_faces", pf=_default_pf(), sky="tex")
    add("sky_none", "sky_faces", pf=_default_pf(), sky="none")
    # bands: partial tile column / row; members deal the frame in bands of 8 rows, a strip starts at row 8 and ends in a cut tile row
    for (w, h) in ((75, 37), (72, 40)):
        for tag, rows in (("2_members", ("members", 2)), ("3_members", ("members", 3)), ("strip", ("range", 8, h - 8 - 3))):
            add(f"bands_{w}x{h}_{tag}", "bands", frame=(w, h), pf=_default_pf(w, h), rows=rows)
    # tiny: the smallest frames that still have a whole tile (8 x 8: one tile in the grid, one thread of the classifier, one wave of the generator) and a cut one (9 x 7: a
    # column of 1 pixel, rows 7 beyond the frame); fovy 20 degrees, so that a tile widened to its full 8 + 2 pixels still looks at one sky face
    add("tiny_8x8_hit", "tiny", frame=(8, 8), pf=_default_pf(8, 8, fovy=20.0), plain=False)
    add("tiny_8x8_empty", "tiny", frame=(8, 8), pf=_default_pf(8, 8, fovy=20.0), scene_kw={"shift": (3.5, 0.0, 0.0)})
    add("tiny_8x8_in_slack", "tiny", frame=(8, 8), pf=_default_pf(8, 8, fovy=20.0), scene_kw={"shift": (2.1875, 0.0, 0.0)}, plain=False)      # at its far end z = -6 the box starts inside pixel column 8: no ray of the frame reaches it, the pixel of slack does
    add("tiny_9x7_whole_hits", "tiny", frame=(9, 7), pf=_default_pf(9, 7, fovy=20.0), scene_kw={"shift": (-0.75, 0.0, 0.0)})              # the box ends in pixel column 5: the cut tile (column 8) is clearly empty
    add("tiny_9x7_cut_hits", "tiny", frame=(9, 7), pf=_default_pf(9, 7, fovy=20.0), scene_kw={"shift": (2.125, 0.0, 0.0)}, plain=False)   # at z = -6 the box starts inside pixel column 8: only the cut tile can hit
    # instances: every walk plan; the gate of 256 instances
    add("inst", "inst", scene="inst", pf=_default_pf(eye=(0.0, 0.0, 4.0)))
    add("inst_needle", "inst", scene="inst", pf=_default_pf(eye=(0.0, 6.0, -294.0), direction=(0.3, -1.0, -0.6)), plain=False)
    add("inst256", "inst", scene="inst256", pf=_default_pf(fovy=40.0, eye=(0.0, 0.0, 0.0)))
    add("inst257", "inst", scene="inst257", pf=_default_pf(fovy=40.0, eye=(0.0, 0.0, 0.0)), expect="zero", plain=False)
    add("same_space", "inst", scene="same_space", pf=_default_pf())
    add("tlas_leaf_root", "inst", scene="tlas_leaf_root", pf=_default_pf(), expect="zero", plain=False)
    add("lights_on", "gates", pf=_default_pf(), lights=True, expect="none", plain=False)
    add("aovs_on", "gates", pf=_default_pf(), aovs=True, expect="zero", plain=False)
    _regressions()
    out += list(REGRESSION_CAMERAS.values())
    return out


CASES = {c.name: c for c in _cases()}
# classes whose every case must hold a sliver: a tile that can hit next to one that cannot (the ref test asserts it)
SLIVER_CLASSES = ("silhouette_on_tile_edge", "edge_on", "near", "lens", "sky_faces")

# walk plans: (developer options, UseTlas); which scenes they apply to
PLANS = {"one_blas": ({}, 0), "loop": ({"inst_tlas": 0, "inst_sieve": 0}, 0), "sieve": ({"inst_tlas": 0, "inst_sieve": 2, "inst_sieve_overlap": 100}, 0),
         "own_tlas": ({"inst_tlas": 8, "inst_tlas_overlap": 100, "inst_unify": 0}, 0), "unified": ({"inst_unify": 4096}, 0), "use_tlas": ({"inst_tlas": 8}, 1)}
COUNTING_PLANS = ("one_blas", "loop", "use_tlas")      # the walks that reproduce the oracle's visit counters
OWN_TREE_PLANS = ("own_tlas", "unified")               # the first boxes are the two root children of the library's own tree over the instances


def plans_of(case):
    if case.scene in ("one", "flat"):
        return ("one_blas", "use_tlas") if case.name.startswith("silhouette_exact") else ("one_blas",)
    if case.scene == "tlas_leaf_root":
        return ("use_tlas",)
    if case.scene == "same_space":
        return ("unified", "loop")
    return ("loop", "sieve", "own_tlas", "use_tlas")


# ----------------------------------------------------------------------------------------------------------------- rows of a context
def local_rows(case, member=0):
    """image rows of the context's local rows, in local order (bands of 8 rows dealt to the members of a group; a strip)"""
    h = case.frame[1]
    if case.rows is None:
        return list(range(h))
    if case.rows[0] == "members":
        return [y for y in range(h) if (y // 8) % case.rows[1] == member]
    return list(range(case.rows[1], min(h, case.rows[1] + case.rows[2])))


# ----------------------------------------------------------------------------------------------------------------- truth (the oracle alone)
class Truth:
    """can_hit[ty, tx], faces[ty, tx] (bit f: some ray of the tile sees sky face f), first[ty, tx] = (pixel x, image row, jitter index, lens index) of the first ray that passes a
    first box test (or None)"""

    def __init__(self, can_hit, faces, first):
        self.can_hit, self.faces, self.first = can_hit, faces, first


def truth(O, case, sc, use_tlas, rows=None):
    L = O.lib()
    w, h = case.frame
    rows = list(range(h)) if rows is None else rows
    tx_n, ty_n = (w + 7) // 8, (len(rows) + 7) // 8
    p = case.pf[0]
    ip = np.ascontiguousarray(p["InvProjection"]); iv = np.ascontiguousarray(p["InvView"]); vp = np.ascontiguousarray(p["ViewPos"])
    lens = LENS if case.radius != 0.0 else LENS[:1]
    d, keep = sc.desc()
    hs = L.ref_scene_create(C.addressof(d))
    can = np.zeros((ty_n, tx_n), bool); faces = np.zeros((ty_n, tx_n), np.uint8); first = np.empty((ty_n, tx_n), object)
    try:
        for ty in range(ty_n):
            for tx in range(tx_n):
                xy = np.int32([(x, rows[ly]) for ly in range(ty * 8, min(ty * 8 + 8, len(rows))) for x in range(tx * 8, min(tx * 8 + 8, w))])
                n = len(xy) * len(JITTERS) * len(lens)
                o = np.zeros((n, 3), np.float32); dr = np.zeros((n, 3), np.float32); fc = np.zeros(n, np.uint8); ps = np.zeros(n, np.uint8)
                L.ref_primary_rays(ip.ctypes.data, iv.ctypes.data, vp.ctypes.data, case.focal, case.radius, w, h, len(xy), xy.ctypes.data, len(JITTERS), JITTERS.ctypes.data,
                                   len(lens), lens.ctypes.data, o.ctypes.data, dr.ctypes.data, fc.ctypes.data)
                L.ref_first_box_tests(hs, int(use_tlas), n, o.ctypes.data, dr.ctypes.data, ps.ctypes.data)
                faces[ty, tx] = np.bitwise_or.reduce(np.uint8(1) << np.unique(fc))
                if ps.any():
                    i = int(np.argmax(ps)); can[ty, tx] = True
                    pi, rest = divmod(i, len(JITTERS) * len(lens)); ji, li = divmod(rest, len(lens))
                    first[ty, tx] = (int(xy[pi, 0]), int(xy[pi, 1]), ji, li)
    finally:
        L.ref_scene_destroy(C.c_void_p(hs)); del keep
    return Truth(can, faces, first)


def describe_ray(first):
    x, y, ji, li = first
    return f"pixel ({x}, {y}) jitter {JITTERS[ji].tolist()!r} lens point {LENS[li].tolist()!r}"


# ----------------------------------------------------------------------------------------------------------------- "clearly empty": the documented rule in binary64, doubled
def _world_dir(ip, iv, nx, ny):
    rx = ip[0] * nx + ip[4] * ny; ry = ip[1] * nx + ip[5] * ny
    v = iv[0, :3] * rx + iv[1, :3] * ry - iv[2, :3]
    return v / np.linalg.norm(v)


def first_boxes(sc, use_tlas, own_tree=False):
    """world-space corners (n, 8, 3), binary64, of the boxes the rule tests: every instance's BLAS root box under its Model rows, or the two children of the TLAS root
    (None: a leaf root or no TLAS — no shortcut).  own_tree: the walk goes through the library's own tree over the instances, whose leaves kernels_scene.hpp documents — the
    world box of each root box under the inverse of InvModel, padded by 2^-10 of its size and of its distance from the origin; the two children of its root lie inside the
    union of the leaves, which stands for them here as ONE box, padded twice as much."""
    def corners(lo, hi):
        return np.float64([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2]] for c in range(8)])
    if own_tree and not use_tlas:
        lo_u, hi_u = np.full(3, np.inf), np.full(3, -np.inf)
        for inst in sc.blas_instances:
            root = sc.blas_nodes[sc.blas_descs[inst["BlasId"]]["NodeOffset"] + 1]
            im = sc.mesh_transforms[inst["MeshTransformId"]]["InvModel"].astype(np.float64)
            wc = (corners(root["Min"].astype(np.float64), root["Max"].astype(np.float64)) - im[:, 3]) @ np.linalg.inv(im[:, :3]).T
            lo, hi = wc.min(0), wc.max(0)
            pad = np.maximum(hi - lo, np.maximum(np.abs(lo), np.abs(hi))) * (2.0 / 1024.0)
            lo_u = np.minimum(lo_u, lo - pad); hi_u = np.maximum(hi_u, hi + pad)
        return corners(lo_u, hi_u)[None]
    if use_tlas:
        if not len(sc.tlas_nodes) or (int(sc.tlas_nodes[0]["IsLeafAndChildOrInstanceId"]) >> 31) == 1:
            return None
        k = int(sc.tlas_nodes[0]["IsLeafAndChildOrInstanceId"]) & 0x7fffffff
        return np.stack([corners(sc.tlas_nodes[k + j]["Min"].astype(np.float64), sc.tlas_nodes[k + j]["Max"].astype(np.float64)) for j in range(2)])
    out = []
    for inst in sc.blas_instances:
        root = sc.blas_nodes[sc.blas_descs[inst["BlasId"]]["NodeOffset"] + 1]
        m = sc.mesh_transforms[inst["MeshTransformId"]]["Model"].astype(np.float64)
        out.append(corners(root["Min"].astype(np.float64), root["Max"].astype(np.float64)) @ m[:, :3].T + m[:, 3])
    return np.stack(out)


def clearly_empty(case, sc, use_tlas, rows=None, factor=2.0, own_tree=False):
    """[ty, tx] bool: the rule k_classify_tiles' comment documents, restated in binary64 with every allowance doubled (factor; 1 is the documented rule itself) — the tile's beam widened by 2 pixels instead of 1, every
    box beyond one side plane of it by more than 2 x the documented margin R + (D + R) * (R / F) * 1.5 + 1e-4 * (D + 1), R = LENS_RIM * r, and, under a constant-per-face sky,
    the four corner directions agreeing on a face by more than 2 x eta = 2 * R / F + 1e-4.  The factor 2 is the allowance for the kernel's binary32 rounding; nothing here comes from the kernel.
    All False where the rule's gate is shut."""
    w, h = case.frame
    rows = list(range(h)) if rows is None else rows
    tx_n, ty_n = (w + 7) // 8, (len(rows) + 7) // 8
    out = np.zeros((ty_n, tx_n), bool)
    r, F = float(f32(case.radius)), float(f32(case.focal))
    boxes = first_boxes(sc, use_tlas, own_tree)
    if boxes is None or not (1 <= len(sc.blas_instances) <= 256) or case.aovs or case.lights or not (r >= 0.0 and f32(F) > f32(1e-3) and f32(r) / f32(F) <= f32(0.05)):      # (the gate is a comparison, stated in the kernel's number format)
        return out
    p = case.pf[0]
    ip = p["InvProjection"].astype(np.float64); iv = p["InvView"].astype(np.float64).reshape(4, 4); apex = p["ViewPos"].astype(np.float64)
    rel = boxes - apex
    D = np.linalg.norm(rel, axis=2).max(1)
    R = LENS_RIM * r
    margin = factor * (R + (D + R) * (R / F) * 1.5 + 1e-4 * (D + 1.0))
    eta = factor * (2.0 * R / F + 1e-4)
    sky_n = 0 if sc.sky_faces is None else sc.sky_faces.shape[1]
    for ty in range(ty_n):
        ys = rows[ty * 8: ty * 8 + 8]
        if ys != list(range(ys[0], ys[0] + len(ys))):
            continue                                     # (cannot happen with bands of 8 rows)
        for tx in range(tx_n):
            nx0, nx1 = (tx * 8 - factor) / w * 2 - 1, (tx * 8 + 8.0 + factor) / w * 2 - 1
            ny0, ny1 = (ys[0] - factor) / h * 2 - 1, (ys[0] + 8.0 + factor) / h * 2 - 1       # (a cut tile is treated as a whole one: wider is stricter)
            u = [_world_dir(ip, iv, nx0, ny0), _world_dir(ip, iv, nx1, ny0), _world_dir(ip, iv, nx1, ny1), _world_dir(ip, iv, nx0, ny1)]
            mid = sum(u)
            ok = True
            for b in range(len(rel)):
                beyond = False
                for i in range(4):
                    n = np.cross(u[i], u[(i + 1) & 3]); ln = np.linalg.norm(n)
                    if ln <= 1e-9:
                        continue
                    n = n / ln
                    if np.dot(n, mid) > 0:
                        n = -n
                    if (rel[b] @ n).min() > margin[b]:
                        beyond = True
                ok = ok and beyond
                if not ok:
                    break
            if ok and sky_n == 1:
                fc = set()
                for v in u:
                    a = np.abs(v); k = int(np.argmax(a)); others = np.delete(a, k)
                    fc.add(2 * k + (0 if v[k] > 0 else 1) if a[k] >= others.max() + eta else -1)
                ok = len(fc) == 1 and -1 not in fc
            out[ty, tx] = ok
    return out
