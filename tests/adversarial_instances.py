"""Adversarial instance sets for the TLAS builders (numpy only, deterministic seeds): equal Morton keys, equal union areas, centres in a plane / on a line / at a point and at
the global maximum, signed zeros in the boxes, instance counts around the device build's thread and chunk boundaries, search radii clamped at both ends, transforms that mirror,
flatten, shear, turn exactly and inexactly and carry far away, and BLASes shared under permuted transform ids.
tests/test_adversarial_instances_ref.py proves on the CPU that each class is what it claims and holds the product's host builder to the oracle on them;
tests/test_gpu_adversarial_instances.py holds the device build (idkptBuildTlasOnDevice) and the frames through it to the oracle.

Every scene is a handful of BLASes of 1-4 triangles (small integer or dyadic vertices: the root boxes are exact) and an instance list over them.  A transform is written as
the 3 x 4 rows the kernels read (Model[k] = (R[k][0], R[k][1], R[k][2], t[k]), world = R c + t): signed zeros and exact entries arrive as written.

Condition on every case (finite_union): all coordinates finite and the binary32 half area of the union of all leaf boxes finite and below FLT_MAX.  The reference's serial
TLAS.Build does not end when no union has a half area below FLT_MAX; with every union area finite a mutual pair exists in every round (the lowest-indexed node of a minimum-area
pair is picked back by its partner under the first-wins rule), so neither the oracle nor the kernel can spin.  Singular transforms appear only as a zero scale on ONE axis (finite,
flat boxes); non-finite ones stay out (tests/test_gpu_inst_tlas.py::test_singular_and_non_finite_transforms_terminate_and_equal_the_loop covers termination there).
"""
import math
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

FLT_MAX = np.float32(3.4028235e+38)
CLASSES = ("same_key", "same_area", "flat", "signed_zero", "counts", "radius", "transforms", "shared_blas")
NZ = np.float32(-0.0)


# ----------------------------------------------------------------------------------------------------------------- BLASes
def _box_tris(lo, hi):
    """Two triangles whose bounds are the box [lo, hi] (every coordinate of a vertex is lo's or hi's, signs of zero included)."""
    (a, b, c), (d, e, f) = lo, hi
    return np.array([[[a, b, c], [d, b, c], [a, e, f]], [[d, e, f], [a, e, c], [d, b, f]]], np.float32)


UNIT = _box_tris((0, 0, 0), (1, 1, 1))
ASYM = _box_tris((-1, -2, -0.5), (2, 1, 4))                         # asymmetric about the origin on every axis
TETRA = np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0]], [[0, 0, 0], [0, 2, 0], [0, 0, 3]], [[0, 0, 0], [0, 0, 3], [2, 0, 0]], [[2, 0, 0], [0, 2, 0], [0, 0, 3]]], np.float32)
FLATX = np.array([[[0, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float32)   # x = 0: a box without extent on one axis
SEGZ = np.array([[[0, 0, 0], [0, 0, 1], [0, 0, 0.5]]], np.float32)  # a segment: no extent on two
POINT = np.zeros((1, 3, 3), np.float32)                              # a point: no extent at all
# x ranges with a zero of either sign at one end; y and z in [1, 2] (strictly positive: a product with a -0 matrix entry is -0 for every corner)
SZ = {"min+": _box_tris((0.0, 1, 1), (1, 2, 2)), "min-": _box_tris((NZ, 1, 1), (1, 2, 2)), "max-": _box_tris((-1, 1, 1), (NZ, 2, 2)), "max+": _box_tris((-1, 1, 1), (0.0, 2, 2)),
      "flat+": _box_tris((0.0, 1, 1), (0.0, 2, 2)), "flat-": _box_tris((NZ, 1, 1), (NZ, 2, 2))}


def _mesh(tp, k):
    p, i, nrm, tan = S.flat_shaded(tp)
    return S.MeshInput(p, i, S.make_material((0.45 + 0.1 * (k % 5), 0.9 - 0.12 * (k % 4), 0.5 + 0.15 * (k % 3), 1.0)), nrm, tan)


# ----------------------------------------------------------------------------------------------------------------- transforms (3 x 4 rows)
def rows(R=None, t=(0.0, 0.0, 0.0)):
    m = np.zeros((3, 4), np.float64)
    m[:, :3] = np.eye(3) if R is None else np.asarray(R, np.float64)
    m[:, 3] = t
    return m


def scale(sx, sy, sz):
    return np.diag([float(sx), float(sy), float(sz)])


def exact_turn(axis, quarters):
    """rotation by quarters * 90 degrees about `axis`: entries 0 and +-1"""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarters % 4]
    m = np.eye(3); u, v = (axis + 1) % 3, (axis + 2) % 3
    m[u, u] = c; m[u, v] = -s; m[v, u] = s; m[v, v] = c
    return m


def turn(axis_vec, deg):
    """Rodrigues: rotation by `deg` about `axis_vec` (sine and cosine rounded)"""
    a = np.asarray(axis_vec, np.float64); a = a / np.linalg.norm(a); x, y, z = a
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    r = math.radians(deg)
    return np.eye(3) + math.sin(r) * K + (1 - math.cos(r)) * (K @ K)


def transforms_of(models):
    """GpuMeshTransform records of 3 x 4 Model rows taken as binary32 AS WRITTEN; InvModel = the inverse in binary64 (all zeros for a singular Model, as a host that hides an
    instance writes it); PrevModel = Model."""
    models = np.asarray(models)
    out = np.zeros(len(models), T.GpuMeshTransform)
    out["Model"] = models.astype(np.float32)
    for i, m in enumerate(out["Model"].astype(np.float64)):
        if abs(np.linalg.det(m[:, :3])) > 1e-30:
            ri = np.linalg.inv(m[:, :3])
            out["InvModel"][i, :, :3] = ri.astype(np.float32); out["InvModel"][i, :, 3] = (-ri @ m[:, 3]).astype(np.float32)
    out["PrevModel"] = out["Model"]
    return out


def make_scene(builder, blases, blas_ids, models, xform_ids=None):
    """blases: triangle arrays (k, 3, 3); instance i = BLAS blas_ids[i] under transform xform_ids[i] (default i) of `models`.  No TLAS is built here."""
    sc = S.assemble([{"meshes": [_mesh(tp, k)]} for k, tp in enumerate(blases)], builder, build_tlas=False)
    inst = np.zeros(len(blas_ids), T.GpuBlasInstance)
    inst["BlasId"] = blas_ids; inst["MeshTransformId"] = np.arange(len(blas_ids)) if xform_ids is None else xform_ids
    sc.blas_instances = inst
    sc.mesh_transforms = models if isinstance(models, np.ndarray) and models.dtype == T.GpuMeshTransform else transforms_of(models)
    return sc


def permuted(sc, seed=1):
    """the transforms after one move: the same records dealt to other slots (a rotation of the slots by a seeded amount, so that every instance moves when n > 1)"""
    n = len(sc.mesh_transforms)
    k = 1 + int(np.random.default_rng(seed).integers(0, max(n - 1, 1))) if n > 1 else 0
    return np.roll(sc.mesh_transforms, k)


# ----------------------------------------------------------------------------------------------------------------- binary32 restatements (numpy)
def _minN(a, b):
    return np.where(a < b, a, b)          # minps: the SECOND operand on a tie (and for +-0)


def _maxN(a, b):
    return np.where(a > b, a, b)


def leaf_boxes(sc):
    """(n, 6) binary32 world boxes of the instances: Box.Transformed (Shapes/Box.cs:177-187) — 8 corners, each coordinate ((cx*m0 + cy*m1) + cz*m2) + 1*m3, grown in corner order"""
    inst = sc.blas_instances
    d = sc.blas_descs[inst["BlasId"]]
    root = sc.blas_nodes[d["NodeOffset"] + 1]
    M = sc.mesh_transforms["Model"][inst["MeshTransformId"]]                 # (n, 3, 4)
    mn = np.full((len(inst), 3), FLT_MAX, np.float32); mx = np.full((len(inst), 3), -FLT_MAX, np.float32)
    for c in range(8):
        p = [np.where((c >> k) & 1, root["Max"][:, k], root["Min"][:, k]).astype(np.float32) for k in range(3)]
        w = np.stack([((p[0] * M[:, k, 0] + p[1] * M[:, k, 1]) + p[2] * M[:, k, 2]) + np.float32(1.0) * M[:, k, 3] for k in range(3)], 1)
        mn = _minN(mn, w); mx = _maxN(mx, w)
    return np.concatenate([mn, mx], 1)


def union_in_order(boxes, order=None):
    """the union of the boxes grown one by one in `order` under the minps / maxps rule (the sign of a zero is the LAST zero's)"""
    mn = np.full(3, FLT_MAX, np.float32); mx = np.full(3, -FLT_MAX, np.float32)
    for i in (range(len(boxes)) if order is None else order):
        mn = _minN(mn, boxes[i, :3]); mx = _maxN(mx, boxes[i, 3:])
    return np.concatenate([mn, mx])


def half_area(mn, mx):
    """fma(sx + sy, sz, sx * sy) (MyMath.cs:222-229): the product and the sum are taken in binary64 (the product of two binary32 numbers is exact there) and rounded once"""
    s = (mx - mn).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((s[..., 0] + s[..., 1]).astype(np.float64) * s[..., 2].astype(np.float64) + s[..., 0].astype(np.float64) * s[..., 1].astype(np.float64)).astype(np.float32)


def finite_union(boxes):
    """the condition on every case; returns the union's half area"""
    assert np.isfinite(boxes).all(), "non-finite leaf coordinate"
    u = union_in_order(boxes)
    a = half_area(u[:3], u[3:])
    assert np.isfinite(a) and a < FLT_MAX and a >= 0, f"union half area {a}"
    return float(a)


def _spread(v):
    v = v.astype(np.uint32)
    for mul, mask in ((0x00010001, 0xFF0000FF), (0x00000101, 0x0F00F00F), (0x00000011, 0xC30C30C3), (0x00000005, 0x49249249)):
        v = ((v.astype(np.uint64) * np.uint64(mul)) & np.uint64(0xFFFFFFFF)).astype(np.uint32) & np.uint32(mask)
    return v


def morton_keys(boxes):
    """(keys, q): the Morton-30 key of every box centre in the union box (MyMath.cs:241-257 MapToZeroOne, :283-299 GetMortonCode30) and its three 10-bit components"""
    g = union_in_order(boxes)
    c = ((boxes[:, 3:] + boxes[:, :3]) * np.float32(0.5)).astype(np.float32)
    ext = (g[3:] - g[:3]).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = ((c - g[:3]) / ext * np.float32(1.0) + np.float32(0.0)).astype(np.float32)
    r = np.where(ext == 0, np.float32(0.0), r)
    f = (r * np.float32(1024.0)).astype(np.float32)
    u = np.where((f != f) | (f <= 0), 0.0, np.minimum(np.floor(f.astype(np.float64)), 4294967295.0))
    q = np.minimum(u, 1023.0).astype(np.uint32)
    return (_spread(q[:, 0]) << np.uint32(2)) | (_spread(q[:, 1]) << np.uint32(1)) | _spread(q[:, 2]), q


def tied_searches(boxes, keys, radius):
    """round 1 of PLOC: the (node, window) searches whose minimum union area is reached by more than one candidate"""
    n = len(boxes)
    b = boxes[np.argsort(keys, kind="stable")]
    best = np.full(n, np.inf); count = np.zeros(n, np.int64)
    for d in [k for k in range(-min(radius, n - 1), min(radius, n - 1) + 1) if k]:
        i = np.arange(max(0, -d), min(n, n - d))
        a = half_area(_minN(b[i, :3], b[i + d, :3]), _maxN(b[i, 3:], b[i + d, 3:])).astype(np.float64)
        lower = a < best[i]; same = a == best[i]
        count[i[lower]] = 1; best[i[lower]] = a[lower]; count[i[same]] += 1
    return int((count > 1).sum())


def census(sc, radius):
    boxes = leaf_boxes(sc)
    keys, q = morton_keys(boxes)
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    g = union_in_order(boxes)
    zero = boxes == 0
    return {"n": len(boxes), "shared_keys": int((cnt[inv] > 1).sum()), "tied_searches": tied_searches(boxes, keys, radius), "zero_extent_axes": int(((g[3:] - g[:3]) == 0).sum()),
            "zeros_pos": int((zero & ~np.signbit(boxes)).sum()), "zeros_neg": int((zero & np.signbit(boxes)).sum()),
            "keys_with_1023": int((q == 1023).any(1).sum()), "keys_with_0": int((q == 0).any(1).sum())}


def first_difference(got, want):
    """where two TLAS node arrays part: the first differing node and which of its eight words"""
    g = np.frombuffer(got.tobytes(), np.uint32).reshape(-1, 8); w = np.frombuffer(want.tobytes(), np.uint32).reshape(-1, 8)
    if g.shape != w.shape:
        return f"{len(g)} nodes for {len(w)}"
    i, k = np.argwhere(g != w)[0]
    return f"node {i} word {k} ({('Min.x', 'Min.y', 'Min.z', 'id', 'Max.x', 'Max.y', 'Max.z', 'pad')[k]}): {g[i, k]:#010x} for {w[i, k]:#010x}"


def leaf_depths(nodes):
    """depth of every leaf of a TLAS node array (root = node 0 at depth 0)"""
    depth = np.zeros(len(nodes), np.int64); out = []
    for i, w in enumerate(nodes["IsLeafAndChildOrInstanceId"]):
        if w >> 31:
            out.append(depth[i])
        else:
            depth[w] = depth[w + 1] = depth[i] + 1
    return np.array(out)


# ----------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, cls, factory, radii, render=False, **claims):
        self.name, self.cls, self.factory, self.radii, self.render, self.claims = name, cls, factory, tuple(radii), render, claims


CASES = {}


def _case(name, cls, radii, render=False, **claims):
    def reg(fn):
        assert name not in CASES and cls in CLASSES
        CASES[name] = Case(name, cls, fn, radii, render, **claims)
        return fn
    return reg


def _at(points):
    return [rows(t=p) for p in points]


# ---- same_key
@_case("coincident_5_of_11", "same_key", (1, 15), render=True)
def _(b):
    pts = [(4, 2, 0)] * 5 + [(0, 0, 0), (9, 0, 3), (2, 7, 1), (8, 8, 8), (0, 5, 6), (6, 1, 7)]
    order = [5, 0, 6, 1, 7, 2, 8, 3, 9, 4, 10]                       # the five coincident ones are not neighbours in the instance list
    return make_scene(b, [UNIT], [0] * 11, _at([pts[i] for i in order]))


@_case("clusters_in_one_cell", "same_key", (1, 2, 15))
def _(b):
    # the union box is [0, 1024]^3: a cell of the key is 1 wide; six centres per cluster inside one cell
    pts = [(0, 0, 0), (1023, 1023, 1023)]
    for base in ((100, 200, 300), (700, 40, 512), (511, 511, 511), (3, 900, 64)):
        pts += [(base[0] + j / 16.0, base[1] + ((5 * j) % 6) / 16.0, base[2] + ((3 * j) % 6) / 16.0) for j in range(6)]
    perm = np.random.default_rng(3).permutation(len(pts))
    return make_scene(b, [UNIT], [0] * len(pts), _at([pts[i] for i in perm]))


@_case("identical_7", "same_key", (1, 2, 15, 7), all_identical=True)
def _(b):
    return make_scene(b, [UNIT], [0] * 7, _at([(0, 0, 0)] * 7))


@_case("identical_1025", "same_key", (15,), all_identical=True)
def _(b):
    return make_scene(b, [UNIT], [0] * 1025, _at([(0, 0, 0)] * 1025))


# ---- same_area
def _lattice(b, dims, seed):
    pts = [(2 * i, 2 * j, 2 * k) for i in range(dims[0]) for j in range(dims[1]) for k in range(dims[2])]
    perm = np.random.default_rng(seed).permutation(len(pts))
    return make_scene(b, [UNIT], [0] * len(pts), _at([pts[i] for i in perm]))


# (ties_from: along a Z curve over two or three axes the two neighbours at distance 1 are never at the same offset, so a window of radius 1 holds no tie there)
_case("lattice_16", "same_area", (1, 2, 15, 16), render=True, ties_from=1)(lambda b: _lattice(b, (16, 1, 1), 1))
_case("lattice_8x8", "same_area", (1, 2, 15, 64), ties_from=2)(lambda b: _lattice(b, (8, 8, 1), 2))
_case("lattice_4x4x4", "same_area", (1, 2, 15, 64), ties_from=2)(lambda b: _lattice(b, (4, 4, 4), 3))


# ---- flat: BLAS 0 carries the grid, BLAS 1 (a point) sits at the union box's maximum corner, so that its centre IS the global maximum on every axis with extent
def _flat(b, blas, pts, corner=None, seed=5):
    ids = [0] * len(pts) + ([1] if corner is not None else [])
    pts = list(pts) + ([corner] if corner is not None else [])
    perm = np.random.default_rng(seed).permutation(len(pts))
    return make_scene(b, [blas, POINT], [ids[i] for i in perm], _at([pts[i] for i in perm]))


_G = [(0, 2 * i, 2 * j) for i in range(5) for j in range(5)]
_case("plane_of_boxes", "flat", (1, 15), zero_axes=0, at_max=True)(lambda b: _flat(b, UNIT, _G, (1, 9, 9)))
_case("plane_of_flats", "flat", (1, 15), render=True, zero_axes=1, at_max=True)(lambda b: _flat(b, FLATX, _G, (0, 9, 9)))
_case("line_of_boxes", "flat", (1, 15), zero_axes=0, at_max=True)(lambda b: _flat(b, UNIT, [(0, 0, 2 * j) for j in range(12)], (1, 1, 23)))
_case("line_of_segments", "flat", (1, 15), zero_axes=2, at_max=True)(lambda b: _flat(b, SEGZ, [(0, 0, 2 * j) for j in range(12)], (0, 0, 23)))
_case("point_of_boxes", "flat", (1, 15), zero_axes=0, at_max=False)(lambda b: _flat(b, UNIT, [(3, 4, 5)] * 9))
_case("point_of_points", "flat", (1, 15), zero_axes=3, at_max=False)(lambda b: _flat(b, POINT, [(3, 4, 5)] * 9))
_case("grid_with_corner_point", "flat", (2, 15), zero_axes=0, at_max=True)(lambda b: _flat(b, UNIT, [(2 * i, 2 * j, 2 * k) for i in range(3) for j in range(3) for k in range(3)], (5, 5, 5)))


# ---- signed_zero: row 0 of every Model is (1, -0, -0, -0): world x = the BLAS's x with its zero's sign; the instances stand in a row along y (distinct keys)
def _signed(b, kinds, order):
    names = list(SZ)
    models = []
    for i in range(len(kinds)):
        m = rows(t=(0, 3 * i, 0)).astype(np.float32)
        m[0] = (1.0, NZ, NZ, NZ)
        models.append(m)
    models = np.array(models, np.float32)
    return make_scene(b, [SZ[k] for k in names], [names.index(kinds[i]) for i in order], models[list(order)])


def _interleaved(n, first):
    """an instance order that is not the spatial one and starts with slot `first`"""
    rest = [i for i in np.random.default_rng(n).permutation(n) if i != first]
    return [first] + rest


_case("zero_min_of_both_signs", "signed_zero", (1, 15), render=True, axis=0, side="Min")(lambda b: _signed(b, ["min+", "min-"] * 6, _interleaved(12, 10)))
_case("zero_max_of_both_signs", "signed_zero", (1, 15), axis=0, side="Max")(lambda b: _signed(b, ["max-", "max+"] * 6, _interleaved(12, 10)))
_case("zero_centres_against_zero_min", "signed_zero", (2, 15), axis=0, side="Min")(lambda b: _signed(b, ["flat-", "min+", "flat+", "min-", "min+", "flat-", "min-", "flat+", "min+", "min-"], _interleaved(10, 8)))


# ---- counts / radius: random boxes, sizes over three decades
def _random(b, n, seed):
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-1.5, 1.5, (n, 3))
    pos = rng.uniform(-50, 50, (n, 3))
    models = [rows(np.diag(size[i]), pos[i]) for i in range(n)]
    return make_scene(b, [UNIT, ASYM], rng.integers(0, 2, n), models)


COUNTS = (1, 2, 3, 4, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000)
for _n in COUNTS:
    # (one fixed seed per n; n = 4 takes the first seed whose tree is not two pairs under a root: with 1004 every round merges everything)
    _case(f"count_{_n}", "counts", (15,), render=_n == 63)(lambda b, n=_n: _random(b, n, 1005 if n == 4 else 1000 + n))
_case("radius_n40", "radius", (1, 2, 3, 15, 39, 40, 4096), render=True)(lambda b: _random(b, 40, 77))
_case("radius_n1025", "radius", (1, 2, 3, 15, 1024, 1025, 4096))(lambda b: _random(b, 1025, 78))


# ---- transforms over ASYM.  Every instance stands at a translation of at least 16 on every axis while the turned / sheared box reaches at most 8 from its origin: the
# world coordinates stay clear of zero, so the roundings of the corner arithmetic stay below one ulp of the result (tests/test_adversarial_instances_ref.py)
def _shear():
    return np.array([[1, 0.5, 0], [0, 1, 0.25], [-0.75, 0, 1]])


TRANSFORM_LIST = [("mirror_x", scale(-1, 1, 1)), ("mirror_xyz", scale(-1, -1, -1)), ("zero_y", scale(1, 0, 1)), ("scale_small_large", scale(2.0 ** -10, 1, 2.0 ** 10)),
                  ("scale_large_small", scale(2.0 ** 10, 2.0 ** -10, 8)), ("shear", _shear())] \
    + [(f"turn{90 * q}_{'xyz'[a]}", exact_turn(a, q)) for a in range(3) for q in (1, 2)] \
    + [("turn23_y", turn((0, 1, 0), 23.0)), ("turn61.3_x", turn((1, 0, 0), 61.3)), ("turn37_123", turn((1, 2, 3), 37.0)), ("turn200_z_mirrored", turn((0, 0, 1), 200.0) @ scale(1, -1, 1))]
MIRRORED = ("mirror_x", "mirror_xyz", "turn200_z_mirrored")


def _transforms(b, far):
    models = []
    for i, (_, R) in enumerate(TRANSFORM_LIST):
        t = np.array([16.0 + 12 * (i % 4), 16.0 + 12 * (i // 4), 16.0 + 3 * (i % 3)])
        if far:
            t[i % 3] = (2.0 ** 20 + 0.37) if i % 2 == 0 else -2.0 ** 20
        models.append(rows(R, t))
    perm = np.random.default_rng(9).permutation(len(models))
    return make_scene(b, [ASYM], [0] * len(models), [models[i] for i in perm])


def transform_names():
    perm = np.random.default_rng(9).permutation(len(TRANSFORM_LIST))
    return [TRANSFORM_LIST[i][0] for i in perm]


_case("transforms_near", "transforms", (1, 15), render=True)(lambda b: _transforms(b, False))
_case("transforms_far", "transforms", (1, 15))(lambda b: _transforms(b, True))


# ---- shared_blas: 3 BLASes, 50 instances; BlasId and MeshTransformId permuted independently, instance order != spatial order
@_case("shared_3_blases_50", "shared_blas", (1, 15, 50), render=True)
def _(b):
    rng = np.random.default_rng(21)
    models = [rows(turn(rng.normal(size=3), rng.uniform(0, 360)) @ np.diag(rng.uniform(0.5, 2.0, 3)), rng.uniform(-12, 12, 3)) for _ in range(50)]
    return make_scene(b, [UNIT, ASYM, TETRA], rng.permutation(np.arange(50) % 3), models, xform_ids=rng.permutation(50))


def bounds_of(sc, builder):
    """leaf bounds by the builder's Box.Transformed, as scenes.rebuild_tlas computes them"""
    out = np.zeros((len(sc.blas_instances), 6), np.float32)
    for i, inst in enumerate(sc.blas_instances):
        off = sc.blas_descs[inst["BlasId"]]["NodeOffset"]
        out[i] = builder.instance_world_bounds(sc.blas_nodes[off + 1: off + 2], sc.mesh_transforms[inst["MeshTransformId"]: inst["MeshTransformId"] + 1])
    return out


def camera_for(boxes, w, h):
    """a camera that looks at the cluster: at the median box centre, from a distance that holds four fifths of the centres in view (a few far or huge boxes do not push it away)"""
    ctr = 0.5 * (boxes[:, :3].astype(np.float64) + boxes[:, 3:])
    c = np.median(ctr, 0)
    d = float(np.percentile(np.linalg.norm(ctr - c, axis=1), 80)) + 3.0
    v = np.array([0.35, 0.45, 1.0]); v /= np.linalg.norm(v)
    return S.Camera(w, h, position=tuple(c + v * d), view_dir=tuple(-v), fovy_deg=60.0)
