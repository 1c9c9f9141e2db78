"""Adversarial scenes and ray classes for the traversal kernels (numpy only, deterministic seeds): zero and subnormal direction components, origins on node planes
(0 * inf = NaN slabs), exact ties on shared edges / vertices / duplicated triangles / a doubled instance, origins on a surface, and MaxDist at, one ulp around and far from
the hit distance.  tests/test_adversarial_rays_ref.py proves on the CPU that each class is what it claims; tests/test_gpu_adversarial_rays.py holds every walk to the oracle on them.

Scenes (idkengine_amd.scenes assembles them):
  lattice             ~1 450 triangles: axis-aligned quads on the dyadic grid k/8 (every coordinate, box plane and shared edge exact in binary32, many node bounds coincide),
                      plus slanted triangles (four of them scene-spanning: PreSplit cuts those in the non-refittable build), zero-area triangles and exact duplicates
  lattice_inst        the same geometry cut into 12 BLASes; 13 instances: every BLAS once, BLAS 3 a second time as instance 4 under instance 3's matrix (every hit on them ties);
                      matrices: identity, exact quarter and half turns (entries 0 and +-1, dyadic translations), one general rotation; instances 11 and 12 stand apart at
                      x = 4 and x = 8, so that a ray can pass between two instances inside the box of a TLAS node that holds both
  lattice_same_space  the 12 BLASes under one InvModel, each used once (the unified tree's case); BLAS 0 and BLAS 11 share six triangles (ties between instances)
  soup                S.soup_scene(3000): random triangles, for the classes whose hits must be robust
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

FLT_MAX = np.float32(3.4028235e+38)
CLASSES = ("axis", "planar", "on_plane", "tiny", "edge", "vertex", "duplicate", "on_surface", "range", "regression")
CID = {n: i for i, n in enumerate(CLASSES)}
RANGE_KINDS = ("T", "below_T", "above_T", "zero", "flt_max", "inf")
PER_CLASS = 1500
N_PARTS = 12
SCENES = ("lattice", "lattice_refit", "lattice_inst", "lattice_same_space", "soup")

# Rays that once exposed a product bug, kept by name (origin, direction, MaxDist); appended to every scene's batch as class "regression".
REGRESSION_RAYS = {
}


# ----------------------------------------------------------------------------------------------------------------- geometry
def _square(axis, p, i, j):
    """The quad (two triangles sharing the diagonal) in the plane x[axis] = p/4 over [i/4, (i+1)/4] x [j/4, (j+1)/4] of the other two axes."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    c = np.zeros((4, 3), np.float32)
    c[:, axis] = p / 4.0
    c[:, u] = np.float32([i, i + 1, i + 1, i]) / 4.0
    c[:, v] = np.float32([j, j, j + 1, j + 1]) / 4.0
    return np.float32([[c[0], c[1], c[2]], [c[0], c[2], c[3]]])


def lattice_parts(seed=7):
    """The lattice as N_PARTS triangle arrays (n, 3, 3) + a dict of what was planted where (triangle rows of the concatenation)."""
    rng = np.random.default_rng(seed)
    cells = [(a, p, i, j) for a in range(3) for p in range(-4, 5) for i in range(-4, 4) for j in range(-4, 4)]
    pick = rng.permutation(len(cells))[:700]
    quads = np.concatenate([_square(*cells[k]) for k in pick])                       # 1 400 triangles, quad q = rows 2q, 2q + 1
    per = (len(pick) // N_PARTS) * 2
    parts = [quads[k * per: (k + 1) * per] if k < N_PARTS - 1 else quads[k * per:] for k in range(N_PARTS)]
    g = lambda lo, hi, n: rng.integers(lo, hi, (n, 3)).astype(np.float32) / np.float32(8.0)      # noqa: E731  (grid points k/8)
    small = []
    while len(small) < 8:
        a = g(-8, 8, 1)[0]; t = np.float32([a, a + g(-2, 3, 1)[0], a + g(-2, 3, 1)[0]])
        if np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) > 0 and (np.abs(np.cross(t[1] - t[0], t[2] - t[0])) > 0).sum() >= 2:
            small.append(t)
    big = np.float32([[[-1, -1, -0.875], [1, -1, -0.75], [0, 1, 0.875]], [[-1, 0.125, -1], [1, 0.25, 1], [-1, 0.375, 1]],
                      [[-0.875, -0.875, 0.75], [0.875, -0.75, -0.75], [0.75, 0.875, 0]], [[1, 1, 1], [-1, 0.5, -0.5], [0.5, -1, -1]]])
    p0 = g(-8, 9, 6)
    zero = np.stack([p0, p0 + np.float32([0.25, 0, 0]), p0 + np.float32([0.5, 0, 0])], 1)      # collinear
    zero[4:, 2] = zero[4:, 0]                                                             # ... and two corners identical
    dup_a = parts[0][:6].copy()                                                            # copies of BLAS 0's first triangles (ties between BLASes when cut)
    dup_b = parts[-1][:6].copy()                                                           # copies of the last part's own (ties inside one BLAS)
    extras = np.concatenate([np.float32(small), big, zero, dup_a, dup_b])
    base = sum(len(p) for p in parts)
    parts[-1] = np.concatenate([parts[-1], extras])
    planted = {"slanted": np.arange(base, base + 12), "zero_area": np.arange(base + 12, base + 18), "dup_of_part0": np.arange(base + 18, base + 24),
               "dup_of_last": np.arange(base + 24, base + 30), "dup_src_part0": np.arange(0, 6), "dup_src_last": np.arange((N_PARTS - 1) * per, (N_PARTS - 1) * per + 6)}
    return parts, planted


def _mesh(tp, k):
    p, i, nrm, tan = S.flat_shaded(tp)
    col = (0.45 + 0.04 * k, 0.9 - 0.05 * k, 0.5 + 0.03 * ((5 * k) % 12), 1.0)
    return S.MeshInput(p, i, S.make_material(col), nrm, tan)


def exact_rotation(axis, quarter_turns):
    """OpenTK-convention 4x4 of a rotation by quarter_turns * 90 degrees about `axis`: entries 0 and +-1, nothing rounded."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarter_turns % 4]
    m = np.eye(4); u, v = (axis + 1) % 3, (axis + 2) % 3
    m[u, u] = c; m[u, v] = s; m[v, u] = -s; m[v, v] = c
    return m


def instance_matrices():
    X, Tr = exact_rotation, S.translation
    m = [np.eye(4), X(1, 1) @ Tr((0.25, 0.0, 0.0)), X(2, 2), X(0, 1) @ Tr((0.0, 0.125, 0.0)), None, S.rotation_y(23.0) @ Tr((0.5, -0.25, 0.0)), Tr((0.125, 0.125, 0.0)),
         X(1, 3), X(0, 2) @ Tr((0.0, 0.0, 0.25)), X(2, 1), np.eye(4), X(1, 2) @ Tr((4.0, 0.0, 0.0)), X(2, 3) @ Tr((8.0, 0.0, 0.0))]
    m[4] = m[3]
    return m


EXACT_INSTANCES = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12)       # every instance of lattice_inst but 5 (the general rotation)
INSTANCE_BLAS = (0, 1, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11)


def lattice(builder, refittable=False):
    parts, _ = lattice_parts()
    return S.assemble([{"meshes": [_mesh(np.concatenate(parts), 0)], "refittable": refittable}], builder)


def lattice_same_space(builder):
    parts, _ = lattice_parts()
    return S.assemble([{"meshes": [_mesh(tp, k)]} for k, tp in enumerate(parts)], builder)


def lattice_inst(builder):
    parts, _ = lattice_parts()
    sc = S.assemble([{"meshes": [_mesh(tp, k)]} for k, tp in enumerate(parts)], builder, build_tlas=False)
    inst = np.zeros(len(INSTANCE_BLAS), T.GpuBlasInstance); inst["BlasId"] = INSTANCE_BLAS; inst["MeshTransformId"] = np.arange(len(INSTANCE_BLAS))
    sc.blas_instances = inst
    sc.mesh_transforms = np.concatenate([S.transform_from_matrix(m) for m in instance_matrices()])
    S.rebuild_tlas(sc, builder)
    return sc


def soup(builder):
    return S.soup_scene(3000, builder, seed=41)


def stale_root_scene(builder):
    """Two instances under the identity for the exact loop's STRICT root test (`t1 < T`, BVHIntersect.glsl:32-39).  Instance 0: a 4 x 4 sheet of quads in the plane z = 1/4.
    Instance 1: sheets in z = 1/4, 0 and -1/4 — root box max z = 1/4 — whose top sheet was then moved to z = 1/2 WITHOUT a refit (a host may do that: the boxes are stale, the
    triangles lie outside them).  A ray coming down the z axis hits instance 0 at T, meets instance 1's root box at t1 == T exactly and — `<` — does not enter it; a walk that
    entered on `<=` would find the moved sheet at a smaller t."""
    sheet = lambda p: np.concatenate([_square(2, p, i, j) for i in range(-2, 2) for j in range(-2, 2)])      # noqa: E731
    sc = S.assemble([{"meshes": [_mesh(sheet(1), 0)]}, {"meshes": [_mesh(np.concatenate([sheet(1), sheet(0), sheet(-1)]), 1)]}], builder)
    d = sc.blas_descs[1]; t = sc.blas_triangles[d["TriangleOffset"]: d["TriangleOffset"] + d["TriangleCount"]]
    ids = np.unique(np.stack([t["X"], t["Y"], t["Z"]], 1))
    pos = sc.vertex_positions.copy()
    top = ids[pos[ids, 2] == 0.25]
    pos[top, 2] = 0.5
    sc.vertex_positions = pos
    return sc


def stale_root_rays(seed=5, n=256):
    """down (and, for contrast, up) the z axis and slightly tilted, from z = 1 / z = -1, off the grid in x / y; MaxDist: FLT_MAX, and T of the hit on instance 0 exactly"""
    rng = np.random.default_rng(seed)
    o = _origins(rng, n, 0.35); o[:, 2] = np.where(np.arange(n) % 4 == 3, -1.0, 1.0)
    d = _signed_zeros(rng, (n, 3)); d[:, 2] = -np.sign(o[:, 2])
    tilt = np.arange(n) % 4 == 2
    d[tilt, 0] = np.float32(2.0 ** -6)
    r = _rays(o, d)
    r["MaxDist"][np.arange(n) % 8 == 1] = np.float32(0.75)
    return r


def make_scene(name, builder):
    return {"lattice": lambda: lattice(builder), "lattice_refit": lambda: lattice(builder, True), "lattice_inst": lambda: lattice_inst(builder),
            "lattice_same_space": lambda: lattice_same_space(builder), "soup": lambda: soup(builder)}[name]()


def world_triangles(sc):
    """(n, 3, 3) float64 world-space corners of the stored BLAS triangles of every instance + (instance, scene-wide triangle id) per row."""
    tris, owner = [], []
    for ii, inst in enumerate(sc.blas_instances):
        d = sc.blas_descs[inst["BlasId"]]
        t = sc.blas_triangles[d["TriangleOffset"]: d["TriangleOffset"] + d["TriangleCount"]]
        p = sc.vertex_positions[np.stack([t["X"], t["Y"], t["Z"]], 1).reshape(-1)].astype(np.float64).reshape(-1, 3, 3)
        m = sc.mesh_transforms[inst["MeshTransformId"]]["Model"].astype(np.float64)
        tris.append(p @ m[:, :3].T + m[:, 3])
        owner.append(np.stack([np.full(len(t), ii), np.arange(len(t)) + d["TriangleOffset"]], 1))
    return np.concatenate(tris), np.concatenate(owner)


# ----------------------------------------------------------------------------------------------------------------- binary32 restatements (numpy float32: one rounding per operation)
def xform34_f32(m, v, w):
    """oracle/ref_math.h xform34: ((r0 * x + r1 * y) + r2 * z) + r3 * w per row, in binary32."""
    m = np.asarray(m, np.float32); v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        return np.stack([((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3] * np.float32(w) for r in range(3)], 1)


def box_slabs_f32(o, d, bmin, bmax):
    """IntersectionRoutines.glsl:25-46 up to the slab products: t0s, t1s of every (ray, box), shape (rays, boxes, 3), in binary32."""
    with np.errstate(all="ignore"):
        inv = (np.float32(1.0) / d.astype(np.float32))[:, None, :]
        return (bmin[None] - o[:, None, :]) * inv, (bmax[None] - o[:, None, :]) * inv


def nan_slab_mask(sc, rays):
    """Per ray: does some node box of the scene's trees give a NaN slab (0 * inf) under the walk's own arithmetic — BLAS nodes with the ray in the instance's space, TLAS nodes with
    the world ray."""
    o, d = rays["Origin"], rays["Direction"]
    out = np.zeros(len(rays), bool)
    for inst in sc.blas_instances:
        de = sc.blas_descs[inst["BlasId"]]
        nodes = sc.blas_nodes[de["NodeOffset"] + 1: de["NodeOffset"] + de["NodeCount"]]
        inv = sc.mesh_transforms[inst["MeshTransformId"]]["InvModel"]
        lo, ld = xform34_f32(inv, o, 1.0), xform34_f32(inv, d, 0.0)
        a, b = box_slabs_f32(lo, ld, nodes["Min"], nodes["Max"])
        out |= np.isnan(a).any((1, 2)) | np.isnan(b).any((1, 2))
    if len(sc.tlas_nodes):
        a, b = box_slabs_f32(o, d, sc.tlas_nodes["Min"], sc.tlas_nodes["Max"])
        out |= np.isnan(a).any((1, 2)) | np.isnan(b).any((1, 2))
    return out


def ray_triangle_f32(o, d, p0, p1, p2):
    """IntersectionRoutines.glsl:6-23 as oracle/ref_math.h states it (cross and dot in GLSL's order, ((x + y) + z)), broadcast over rays x triangles in binary32.
    Returns (accepted, t)."""
    f = np.float32
    def cross(a, b):
        return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0], a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)
    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    with np.errstate(all="ignore"):
        p1p0 = (p1 - p0)[None]; p2p0 = (p2 - p0)[None]; rop0 = o[:, None, :] - p0[None]
        n = cross(p1p0, p2p0); q = cross(rop0, d[:, None, :])
        inv = f(1.0) / dot(d[:, None, :], n)
        t = dot(-n, rop0) * inv; by = dot(-q, p2p0) * inv; bz = dot(q, p1p0) * inv
        bx = f(1.0) - by - bz
        return (bx >= 0) & (by >= 0) & (bz >= 0) & (t >= 0), t


def closest_ties(sc, rays, chunk=256, by_value=False):
    """Per ray: how many (instance, triangle) candidates the triangle test accepts at the bits of the smallest accepted T below MaxDist (0 = no hit); tests/test_oracle_rayquery.py
    brute_force_closest vectorised.  by_value: at the VALUE of that T (-0 and +0 tie: `t < T` compares values)."""
    out = np.zeros(len(rays), np.int64)
    for lo_ in range(0, len(rays), chunk):
        r = rays[lo_: lo_ + chunk]
        ts = []
        for inst in sc.blas_instances:
            de = sc.blas_descs[inst["BlasId"]]
            t = sc.blas_triangles[de["TriangleOffset"]: de["TriangleOffset"] + de["TriangleCount"]]
            inv = sc.mesh_transforms[inst["MeshTransformId"]]["InvModel"]
            lo, ld = xform34_f32(inv, r["Origin"], 1.0), xform34_f32(inv, r["Direction"], 0.0)
            ok, tt = ray_triangle_f32(lo, ld, sc.vertex_positions[t["X"]], sc.vertex_positions[t["Y"]], sc.vertex_positions[t["Z"]])
            ts.append(np.where(ok & (tt < r["MaxDist"][:, None]), tt, np.float32(np.inf)))
        ts = np.concatenate(ts, 1)
        best = ts.min(1)
        same = (ts == best[:, None]) if by_value else (ts.view(np.uint32) == best.view(np.uint32)[:, None])
        out[lo_: lo_ + chunk] = np.where(np.isfinite(best), same.sum(1), 0)
    return out


# ----------------------------------------------------------------------------------------------------------------- ray classes
def _rays(o, d, max_dist=FLT_MAX):
    r = np.zeros(len(o), T.RayQuery)
    r["Origin"] = np.asarray(o, np.float32); r["Direction"] = np.asarray(d, np.float32); r["MaxDist"] = max_dist
    return r


def _signed_zeros(rng, shape):
    return np.where(rng.integers(0, 2, shape) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)


def _origins(rng, n, scale):
    """Off the dyadic grid: k/8 + (1, 2, 3)/32 + noise per axis (the three offsets differ so that an axis ray does not meet a quad on its diagonal), times `scale`."""
    k = rng.integers(-10, 10, (n, 3)) / 8.0
    return ((k + np.float64([1, 2, 3]) / 32.0 + rng.uniform(-1 / 256.0, 1 / 256.0, (n, 3))) * scale).astype(np.float32)


def _axis_dirs(rng, n):
    d = _signed_zeros(rng, (n, 3)); ax = rng.integers(0, 3, n)
    d[np.arange(n), ax] = rng.choice(np.float32([-1.0, 1.0]), n)
    return d, ax


def _planar_dirs(rng, n):
    """one component exactly +-0, the other two random; normalised in binary64, then rounded: the zero stays zero"""
    v = rng.normal(size=(n, 3)); z = rng.integers(0, 3, n)
    v[np.arange(n), z] = 0.0
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    d = v.astype(np.float32)
    d[np.arange(n), z] = _signed_zeros(rng, n)
    return d, z


def _through(rng, d, targets, scale):
    """origins of rays with directions d: off the grid, or — `targets`: points the rays are to pass (a sparse scene) — a random distance in front of a target"""
    if targets is None:
        return _origins(rng, len(d), scale)
    return (targets - d.astype(np.float64) * rng.uniform(0.05, 0.8, (len(d), 1)) * scale).astype(np.float32)


def interior_points(rng, sc, n):
    """random points well inside random triangles of the scene (every barycentric >= 0.15), world space, binary64"""
    tris, _ = world_triangles(sc)
    t = tris[rng.integers(0, len(tris), n)]
    b = 0.15 + 0.55 * rng.dirichlet((1.0, 1.0, 1.0), n)
    return (t * b[:, :, None]).sum(1)


def gen_axis(rng, n, scale, targets=None):
    d, _ = _axis_dirs(rng, n)
    return _rays(_through(rng, d, targets, scale), d)


def gen_planar(rng, n, scale, targets=None):
    d, _ = _planar_dirs(rng, n)
    return _rays(_through(rng, d, targets, scale), d)


def gen_tiny(rng, n, scale, targets=None):
    """one component subnormal (1/x = inf, x != 0), at 1e-30 (1/x finite and huge) or at 4e-39 (subnormal, 1/x = 2.5e38 still finite: the slab product overflows from a distance of 1.36 on); the others random"""
    v = rng.normal(size=(n, 3)); z = rng.integers(0, 3, n)
    v[np.arange(n), z] = 0.0
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    d = v.astype(np.float32)
    mag = np.float32([1e-40, 1e-30, 4e-39, 1.4e-45])[np.arange(n) % 4]
    d[np.arange(n), z] = mag * rng.choice(np.float32([-1.0, 1.0]), n)
    return _rays(_through(rng, d, targets, scale), d)


def _node_table(sc):
    """(instance or -1 for the TLAS, Min, Max) of every box a walk can test"""
    rows = []
    for ii, inst in enumerate(sc.blas_instances):
        de = sc.blas_descs[inst["BlasId"]]
        for nd in sc.blas_nodes[de["NodeOffset"] + 1: de["NodeOffset"] + de["NodeCount"]]:
            rows.append((ii, nd["Min"], nd["Max"]))
    for nd in sc.tlas_nodes:
        rows.append((-1, nd["Min"], nd["Max"]))
    return rows


def gen_on_plane(rng, n, sc, exact_instances=None):
    """axis / planar rays that start inside a node box, ON one of its planes along an axis whose direction component is zero: (bound - origin) * (1 / 0) = 0 * inf = NaN in that slab.
    Instanced scenes: the box is a BLAS node of an instance whose matrix is exact (0, +-1, dyadic translation), and origin and direction are mapped to world space — exactly where
    it matters: the coordinate on the plane — or a TLAS node with the world ray."""
    table = _node_table(sc)
    if exact_instances is not None:
        table = [t for t in table if t[0] == -1 or t[0] in exact_instances]
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    da, aa = _axis_dirs(rng, n); dp, zp = _planar_dirs(rng, n)
    for i in range(n):
        ii, lo, hi = table[rng.integers(0, len(table))]
        planar = i % 2 == 1
        ld = dp[i] if planar else da[i]
        zero_axes = [int(zp[i])] if planar else [a for a in range(3) if a != aa[i]]
        p = (lo + (hi - lo) * rng.uniform(0.05, 0.95, 3).astype(np.float32)).astype(np.float32)
        on = zero_axes if (not planar and i % 4 == 0) else [zero_axes[rng.integers(0, len(zero_axes))]]
        for a in on:
            p[a] = lo[a] if rng.integers(0, 2) else hi[a]
        if ii >= 0:
            m = sc.mesh_transforms[sc.blas_instances[ii]["MeshTransformId"]]["Model"].astype(np.float64)       # 3x4: world = M[:, :3] @ p + M[:, 3]
            p = (m[:, :3] @ p.astype(np.float64) + m[:, 3]).astype(np.float32); ld = (m[:, :3] @ ld.astype(np.float64)).astype(np.float32)
        o[i] = p; d[i] = ld
    return _rays(o, d)


def _grid_features(parts):
    """Shared edges and vertices of the lattice's quads, per orientation: {(axis, p, edge or vertex key): number of quads that touch it}"""
    quads = np.concatenate(parts[:N_PARTS])[: 1400].reshape(-1, 2, 3, 3)
    edges, verts = {}, {}
    for q in quads:
        c = np.concatenate([q[0], q[1][2:]])                 # the four corners
        axis = int(np.argmax(np.ptp(c, 0) == 0)); u, v = (axis + 1) % 3, (axis + 2) % 3
        p = c[0, axis]; u0, v0 = c[:, u].min(), c[:, v].min()
        for e in (("u", u0, v0), ("u", u0, v0 + 0.25), ("v", u0, v0), ("v", u0 + 0.25, v0)):      # the edge along u / v that starts at (.., ..)
            edges[(axis, p) + e] = edges.get((axis, p) + e, 0) + 1
        for du in (0.0, 0.25):
            for dv in (0.0, 0.25):
                verts[(axis, p, u0 + du, v0 + dv)] = verts.get((axis, p, u0 + du, v0 + dv), 0) + 1
    return quads, edges, verts


def _aimed(rng, targets, axes):
    """direction +-e_axis, origin on the lattice k/16 in front of the target: every coordinate dyadic, T exact"""
    n = len(targets)
    d = _signed_zeros(rng, (n, 3)); sgn = rng.choice(np.float32([-1.0, 1.0]), n)
    d[np.arange(n), axes] = sgn
    dist = (rng.choice([1, 3], n) + 4 * (rng.integers(0, 4, n) == 0) * rng.integers(0, 3, n)) / 16.0
    o = np.asarray(targets, np.float64).copy()
    o[np.arange(n), axes] -= sgn * dist
    return _rays(o.astype(np.float32), d)


def gen_edge(rng, n, parts):
    """aimed at a point of an edge two triangles share: the diagonal of a quad, or the grid edge between two quads of one plane"""
    quads, edges, _ = _grid_features(parts)
    shared = [k for k, c in edges.items() if c >= 2]
    tg = np.zeros((n, 3)); ax = np.zeros(n, np.int64)
    for i in range(n):
        if i % 2 == 0:
            q = quads[rng.integers(0, len(quads))]; a, c = q[0][0].astype(np.float64), q[0][2].astype(np.float64)      # the diagonal runs from corner 0 to corner 2
            tg[i] = a + (c - a) * (rng.integers(1, 8) / 8.0); ax[i] = int(np.argmax(a == c))
        else:
            axis, p, along, u0, v0 = shared[rng.integers(0, len(shared))]
            u, v = (axis + 1) % 3, (axis + 2) % 3
            s = rng.uniform(0.02, 0.23) if i % 4 == 1 else rng.integers(1, 8) / 32.0
            tg[i, axis] = p; tg[i, u] = u0 + (s if along == "u" else 0.0); tg[i, v] = v0 + (s if along == "v" else 0.0); ax[i] = axis
    return _aimed(rng, np.float32(tg), ax)


def gen_vertex(rng, n, parts):
    """aimed at a grid vertex that two to four quads of one plane touch (two to six triangles)"""
    _, _, verts = _grid_features(parts)
    shared = [k for k, c in verts.items() if c >= 2]
    tg = np.zeros((n, 3)); ax = np.zeros(n, np.int64)
    for i in range(n):
        axis, p, uu, vv = shared[rng.integers(0, len(shared))]
        tg[i, axis] = p; tg[i, (axis + 1) % 3] = uu; tg[i, (axis + 2) % 3] = vv; ax[i] = axis
    return _aimed(rng, np.float32(tg), ax)


def _toward(rng, pts, scale, axis_share=0.5):
    """rays that end up on pts: half of them along +-e_i from a dyadic distance, half from a random direction"""
    n = len(pts)
    d, ax = _axis_dirs(rng, n)
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    rnd = rng.uniform(0, 1, n) >= axis_share
    d[rnd] = v[rnd].astype(np.float32)
    dist = np.where(rnd, rng.uniform(0.05, 0.6, n) * scale, rng.choice([1, 3, 5], n) / 16.0)
    return _rays((np.asarray(pts, np.float64) - d.astype(np.float64) * dist[:, None]).astype(np.float32), d)


def gen_duplicate(rng, n, sc, tri_rows, scale=1.0):
    """aimed at interior points (dyadic barycentrics) of the world-space triangles `tri_rows` of world_triangles(sc): every hit there has a twin at the same T"""
    tris, _ = world_triangles(sc)
    t = tris[np.asarray(tri_rows)[rng.integers(0, len(tri_rows), n)]]
    b = np.float64([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5], [0.625, 0.125, 0.25]])[rng.integers(0, 4, n)]
    return _toward(rng, (t * b[:, :, None]).sum(1), scale)


def gen_on_surface(rng, n, parts):
    """origin exactly ON a quad's triangle — an interior point, a point of an edge, a vertex: t == 0 is a hit (t >= 0) —, direction in the triangle's plane (dot(rd, n) == 0:
    invDet infinite) or out of it"""
    quads, _, _ = _grid_features(parts)
    o = np.zeros((n, 3)); d = np.zeros((n, 3), np.float32)
    da, _ = _axis_dirs(rng, n); dp, _ = _planar_dirs(rng, n)
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    for i in range(n):
        q = quads[rng.integers(0, len(quads))]; c = np.concatenate([q[0], q[1][2:]]).astype(np.float64)
        axis = int(np.argmax(np.ptp(c, 0) == 0)); u, vv = (axis + 1) % 3, (axis + 2) % 3
        where = i % 3
        du, dv = [(rng.integers(1, 4) / 16.0, rng.integers(1, 4) / 16.0 + 1 / 32.0), (rng.integers(1, 8) / 32.0, 0.0), (0.0, 0.0)][where]
        o[i] = c[0]; o[i, u] = c[:, u].min() + du; o[i, vv] = c[:, vv].min() + dv
        kind = (i // 3) % 4
        if kind == 0:                                   # in the plane, along an axis
            d[i] = 0.0; d[i, u if rng.integers(0, 2) else vv] = rng.choice([-1.0, 1.0])
        elif kind == 1:                                 # in the plane, any direction
            w = v[i].copy(); w[axis] = 0.0; w /= np.linalg.norm(w); d[i] = w.astype(np.float32)
        elif kind == 2:                                 # along the normal
            d[i] = 0.0; d[i, axis] = rng.choice([-1.0, 1.0])
        else:
            d[i] = v[i].astype(np.float32)
    return _rays(o.astype(np.float32), d)


def gen_range(base, hits, n):
    """rays of `base` that hit at T (the oracle's `hits`) with MaxDist = T, the float below, the float above, 0, FLT_MAX, +inf in turn; returns (rays, kind per ray)"""
    idx = np.nonzero((hits["Hit"] != 0) & (hits["TriangleId"] != 0xFFFFFFFF) & (hits["T"] > 0))[0][:n]
    r = base[idx].copy(); t = hits["T"][idx].astype(np.float32)
    kind = np.arange(len(idx)) % 6
    md = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [t, np.nextafter(t, np.float32(0.0)), np.nextafter(t, np.float32(np.inf)), np.float32(0.0), FLT_MAX], np.float32(np.inf))
    r["MaxDist"] = md.astype(np.float32)
    return r, kind


def make_rays(name, sc, trace, seed=11):
    """The batch of scene `name`: (rays, class id per ray, range kind per ray or -1).  trace(rays) -> RayHit array is the oracle's closest-hit query (the class `range` needs the
    hit distances).  ~1 500 rays per class, classes in CLASSES order, then the named regression rays."""
    rng = np.random.default_rng(seed + SCENES.index(name))
    n = PER_CLASS
    scale = 10.0 if name == "soup" else 1.0
    tg = (lambda: interior_points(rng, sc, n)) if name == "soup" else (lambda: None)      # the soup is sparse: its rays are sent through its triangles
    out = [("axis", gen_axis(rng, n, scale, tg())), ("planar", gen_planar(rng, n, scale, tg())),
           ("on_plane", gen_on_plane(rng, n, sc, EXACT_INSTANCES if name == "lattice_inst" else None)), ("tiny", gen_tiny(rng, n, scale, tg()))]
    if name != "soup":
        parts, planted = lattice_parts()
        out += [("edge", gen_edge(rng, n, parts)), ("vertex", gen_vertex(rng, n, parts))]
        if name == "lattice_inst":
            # the doubled instance: world-space rows of instances 3 and 4 — and, inside the last BLAS, the planted copies
            _, owner = world_triangles(sc)
            rows = np.nonzero(np.isin(owner[:, 0], (3, 4)))[0]
            last = sc.blas_descs[N_PARTS - 1]
            rows = np.concatenate([rows, np.nonzero((owner[:, 0] == 12) & (owner[:, 1] >= last["TriangleOffset"] + last["TriangleCount"] - 6))[0]])
            out.append(("duplicate", gen_duplicate(rng, n, sc, rows)))
        else:
            # aimed at the sources of the planted copies, in world space = lattice space (identity transforms)
            tp = np.concatenate(parts).astype(np.float64)
            src = np.concatenate([planted["dup_src_part0"], planted["dup_src_last"]])
            t = tp[src[rng.integers(0, len(src), n)]]
            b = np.float64([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5], [0.625, 0.125, 0.25]])[rng.integers(0, 4, n)]
            out.append(("duplicate", _toward(rng, (t * b[:, :, None]).sum(1), 1.0)))
        out.append(("on_surface", gen_on_surface(rng, n, parts)))
    base = np.concatenate([r for _, r in out])
    base = base[np.random.default_rng(seed).permutation(len(base))]
    rr, kind = gen_range(base, trace(base), n)
    rays = np.concatenate([r for _, r in out] + [rr])
    cls = np.concatenate([np.full(len(r), CID[c]) for c, r in out] + [np.full(len(rr), CID["range"])])
    kinds = np.concatenate([np.full(len(rays) - len(rr), -1), kind])
    if REGRESSION_RAYS:
        reg = _rays([v[0] for v in REGRESSION_RAYS.values()], [v[1] for v in REGRESSION_RAYS.values()], np.float32([v[2] for v in REGRESSION_RAYS.values()]))
        rays = np.concatenate([rays, reg]); cls = np.concatenate([cls, np.full(len(reg), CID["regression"])]); kinds = np.concatenate([kinds, np.full(len(reg), -1)])
    return rays, cls, kinds


def batches(rays, cls, seed=3):
    """The batch itself and the ragged ones: 4 099, 65, 63 and 1 rays drawn across all classes (index arrays into the batch)."""
    perm = np.random.default_rng(seed).permutation(len(rays))
    return {"all": np.arange(len(rays)), "4099": perm[:4099], "65": perm[4099:4164], "63": perm[4164:4227], "1": perm[4227:4228]}


def describe(rays, cls, kinds, i):
    r = rays[i]
    return f"ray {i}: class {CLASSES[cls[i]]}{'' if kinds[i] < 0 else '/' + RANGE_KINDS[kinds[i]]} origin {r['Origin'].tolist()!r} direction {r['Direction'].tolist()!r} MaxDist {float(r['MaxDist'])!r}"


def first_difference(got, want, rays, cls, kinds):
    """None, or the report of the first ray whose RayHit differs: class, origin, direction, the first differing field with both values"""
    if got.tobytes() == want.tobytes():
        return None
    g = np.frombuffer(got.tobytes(), np.uint32).reshape(len(got), -1); w = np.frombuffer(want.tobytes(), np.uint32).reshape(len(want), -1)
    i = int(np.nonzero((g != w).any(1))[0][0])
    for f in got.dtype.names:
        if got[f][i].tobytes() != want[f][i].tobytes():
            return f"{describe(rays, cls, kinds, i)}: field {f} is {got[f][i]!r}, the oracle has {want[f][i]!r}; {int((g != w).any(1).sum())} rays differ"
    return f"{describe(rays, cls, kinds, i)}: differs"


# ----------------------------------------------------------------------------------------------------------------- cameras of the path-tracer cases (raw per-frame data)
def perframe(kind, inv_view=None, view_pos=(0.0, 0.0, 0.0), fov=1.0):
    """(InvProjection[16], InvView[16], ViewPos[3]) as float32, OpenTK memory order.  "parallel": InvProjection[0], [1], [4], [5] = 0 -> every primary ray is the -Z column of
    InvView exactly, whatever the jitter.  "planar": [0] and [4] = 0 -> dir.x == 0 exactly while y / z fan out (pt_device.hpp GetWorldSpaceDirection: rx = ip[0] * nx + ip[4] * ny)."""
    ip = np.zeros(16, np.float32)
    ip[10] = 0.0; ip[11] = -1.0; ip[14] = -1.0; ip[15] = 1.0        # (only [0], [1], [4], [5] reach the ray direction)
    if kind == "planar":
        ip[5] = fov; ip[1] = 0.25 * fov
    elif kind != "parallel":
        raise ValueError(kind)
    iv = np.eye(4, dtype=np.float32) if inv_view is None else np.asarray(inv_view, np.float32)
    iv = iv.copy().reshape(4, 4); iv[3, :3] = view_pos
    p = np.zeros(1, T.GpuPerFrameData)
    p["InvProjection"][0] = ip; p["InvView"][0] = iv.reshape(16); p["ViewPos"][0] = view_pos
    return p


def rare_plane(sc, axis=0):
    """A coordinate along `axis` that is a bound of a few BLAS nodes only (an odd multiple of 1/8: the quads lie on multiples of 1/4, the slanted triangles do not): a ray in that
    plane meets NaN slabs at those nodes while the boxes above them straddle the plane — it still reaches geometry.  (A ray in a plane that many boxes share is dropped by the
    boxes on both sides of it, IntersectionRoutines.glsl:25-46, and sees nothing.)"""
    v = np.concatenate([sc.blas_nodes["Min"][:, axis], sc.blas_nodes["Max"][:, axis]])
    v = v[(np.abs(v) < 0.9) & (v * 8 == np.round(v * 8)) & (np.round(v * 8) % 2 == 1)]
    vals, counts = np.unique(v, return_counts=True)
    return float(vals[np.argmax(counts)])


def primary_direction(per_frame):
    """The direction of every primary ray of a "parallel" record: normalize(InvView * (0, 0, -1, 0)) in binary32 (pt_device.hpp GetWorldSpaceDirection with rx = ry = 0)."""
    iv = per_frame["InvView"][0].astype(np.float32); z = np.float32(0.0); m1 = np.float32(-1.0)
    v = np.float32([((iv[k] * z + iv[4 + k] * z) + iv[8 + k] * m1) + iv[12 + k] * z for k in range(3)])
    inv = np.float32(1.0) / np.sqrt(np.float32((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
    return (v * inv).astype(np.float32)
