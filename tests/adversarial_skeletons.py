"""Adversarial SKELETONS for idkptSkin (k_skin) and the refit that follows it (k_refit_leaves / k_refit_level): deterministic, numpy + idkengine_amd.scenes only.
Every case sits ON an edge of the skinning arithmetic instead of inside an interval; tests/skin_ref.py says what the device must store for it, byte for byte.
tests/test_skin_ref.py proves on the CPU that each case is the edge it was built for (its intermediate really is NaN / Inf / a .5 tie / out of range);
tests/test_gpu_adversarial_skeletons.py holds the device to the restatement on every case and checks that every `refused` case is refused before any launch.

A case is a dict: name, cls, un (GpuUnskinnedVertex table, <= 130 entries), joints (J, 3, 4), args = (input_offset, output_offset, joint_offset, count), main (vertices of
the skinned mesh), geometry, tags, refused (None, "joint" or "range"), joints2 (a second joint table: the same range is skinned twice).

The scene of a case (scene(case, builder)): BLAS 0 is a pad of PAD = 12 vertices / 4 triangles that nothing skins, BLAS 1 the skinned mesh, refittable, `main` vertices —
so every refit after a skin runs on a BlasId > 0 with non-zero node, triangle and vertex offsets.  The scene's vertex table holds PAD + main vertices; offsets in `args`
address that table.  Geometries of BLAS 1: "strip" (triangle k = vertices k, k + 1, k + 2), "one_triangle" (the root is duplicated into nodes 2 and 3), "fat_leaf"
(triangles that share one box: the builder cannot split them, a leaf holds several).

Kept out, and why: non-finite positions into the refit (min / max of NaN boxes has no pinned rule in the reference's shader; the restatement, not the device, picks the cases
whose skinned positions are finite and only those are refitted); vertex tables beyond 130 entries (nothing in k_skin depends on the index beyond the guard and the offsets)."""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402

f32 = np.float32
CLASSES = ("weights", "joints", "codes", "indices", "ranges", "refit", "refused")
PAD = 12
FLT_MAX = float(np.finfo(f32).max)
INF, NAN = float("inf"), float("nan")
NZ = -0.0
MID_HI = 1024 | (1024 << 11) | (512 << 22)       # the codes just above the middle of every field
MID_LO = 1023 | (1023 << 11) | (511 << 22)       # ... and just below


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _dyadic(rng, shape, span=2.0, bits=6):
    return (rng.integers(-int(span * 2 ** bits), int(span * 2 ** bits) + 1, shape) / 2.0 ** bits).astype(f32)


def _unit(rng, n):
    v = rng.normal(0, 1, (n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(f32)


def verts(n, seed, indices=(0, 1, 0, 1), weights=(0.5, 0.25, 0.125, 0.125)):
    """n unskinned vertices: dyadic positions in [-2, 2], random unit normals / tangents, the same indices and weights everywhere"""
    rng = _rng(seed)
    un = np.zeros(n, T.GpuUnskinnedVertex)
    un["Position"] = _dyadic(rng, (n, 3))
    un["Normal"] = S.compress_sr11g11b10(_unit(rng, n)); un["Tangent"] = S.compress_sr11g11b10(_unit(rng, n))
    un["JointIndices"] = np.uint32(indices); un["JointWeights"] = f32(weights)
    return un


def affine(linear, translation=(0.0, 0.0, 0.0)):
    j = np.zeros((3, 4), f32); j[:, :3] = np.asarray(linear, np.float64).astype(f32); j[:, 3] = f32(translation)
    return j


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def generic_joints():
    """two finite, well-conditioned joints: a translation and a turn"""
    return np.stack([affine(np.eye(3), (0.125, 0.0, -0.25)), affine(rot_y(0.3) @ rot_x(-0.2), (0.0, 0.375, 0.0))])


def _case(name, cls, un, joints, args=None, main=None, geometry="strip", tags=(), refused=None, joints2=None):
    joints = np.ascontiguousarray(joints, f32).reshape(-1, 3, 4)
    if args is None:
        args = (0, PAD, 0, len(un))
    if main is None:
        main = max(args[3], 3) + 5                      # the range never covers the whole mesh unless a case says so: writes past it would show
    assert len(un) <= 130
    return dict(name=name, cls=cls, un=un, joints=joints, args=tuple(int(a) for a in args), main=int(main), geometry=geometry, tags=frozenset(tags), refused=refused,
                joints2=None if joints2 is None else np.ascontiguousarray(joints2, f32).reshape(-1, 3, 4))


def _tie_down_case():
    """Ties whose EVEN neighbour is the lower one (k + 0.5 with k even): rint gives k, floor(x + 0.5) gives k + 1.  u * 2047 is itself rounded to binary32, so a product that
    is exactly k + 0.5 exists for about one scale in 2^14; a deterministic scan over the scale s of diag(1, s, 1) (y field, 2047) and diag(1, 1, s) (z field, 1023) on one fixed
    normal finds them, with the very arithmetic of tests/skin_ref.py.  Each hit becomes one joint and one vertex."""
    import skin_ref as R
    word = np.uint32(1500 | (1300 << 11) | (700 << 22))
    v = R.decompress(np.array([word]))[0]
    s = (f32(0.25) + np.arange(1 << 22, dtype=f32) * f32(2.0 ** -21)).astype(f32)
    joints = []
    for axis, mask in ((1, 2047), (2, 1023)):
        t = np.tile(v, (len(s), 1)).astype(f32); t[:, axis] = (s * v[axis]).astype(f32)
        n, _, _ = R.normalize(t)
        x = ((n[:, axis] * f32(0.5) + f32(0.5)) * f32(mask)).astype(f32)
        hit = np.nonzero((x - np.floor(x) == 0.5) & (np.floor(x) % 2 == 0))[0][:16]
        assert len(hit) >= 8, (axis, len(hit))
        for h in hit:
            d = np.ones(3); d[axis] = float(s[h]); joints.append(affine(np.diag(d)))
    un = verts(len(joints), 22, indices=(0, 0, 0, 0), weights=(1, 0, 0, 0))
    un["JointIndices"][:, 0] = np.arange(len(joints)); un["Normal"] = word; un["Tangent"] = word
    return _case("j_tie_to_the_even_code_below", "joints", un, joints, tags=("tie_down",))


def _cases():
    out = []
    G = generic_joints()
    # ------------------------------------------------------------------------------------------------------------------ weights
    out.append(_case("w_all_zero", "weights", verts(65, 1, weights=(0, 0, 0, 0)), G, tags=("nan_vector",)))                      # M = 0: normalize(0) = 0 * (1 / 0) = NaN
    inf_j = np.concatenate([G[:1], np.full((3, 3, 4), INF, f32)])
    out.append(_case("w_one_hot_inf_unused", "weights", verts(65, 2, indices=(0, 1, 2, 3), weights=(1, 0, 0, 0)), inf_j, tags=("nan_vector", "nan_position")))   # 0 * Inf = NaN
    out.append(_case("w_sum_quarter", "weights", verts(65, 3, weights=(0.0625, 0.0625, 0.0625, 0.0625)), G))
    out.append(_case("w_sum_four", "weights", verts(65, 4, weights=(1, 1, 1, 1)), G))
    out.append(_case("w_negative", "weights", verts(65, 5, weights=(1.5, -0.5, 0.25, -0.25)), G))
    out.append(_case("w_cancel", "weights", verts(65, 6, indices=(1, 1, 0, 0), weights=(0.75, -0.75, 0, 0)), G, tags=("nan_vector", "zero_matrix")))   # w a + (-w a) == 0 exactly
    out.append(_case("w_subnormal", "weights", verts(65, 7, weights=(1e-40, 1e-40, 0, 0)), G, tags=("inf_vector",)))           # |t| ~ 1e-40: dot underflows to 0, t * (1 / 0)
    un = verts(65, 8); un["JointWeights"][::3, 2] = NAN
    out.append(_case("w_nan", "weights", un, G, tags=("nan_vector", "nan_position")))
    # ------------------------------------------------------------------------------------------------------------------ joints
    one = dict(indices=(0, 0, 0, 0), weights=(1, 0, 0, 0))
    two = dict(indices=(0, 1, 0, 1), weights=(1, 0, 0, 0))
    out.append(_case("j_identity", "joints", verts(65, 10, **one), [affine(np.eye(3))]))
    out.append(_case("j_mirror", "joints", verts(129, 11, **one), [affine(np.diag([-1.0, 1.0, 1.0]) @ rot_y(0.4), (0.25, 0.0, 0.0))], tags=("frame",)))
    out.append(_case("j_nonuniform", "joints", verts(129, 12, **one), [affine(rot_x(0.3) @ np.diag([1e3, 4e2, 1e-3]) / 500.0, (0.0, 0.5, 0.0))], tags=("frame",)))
    un = verts(66, 13, **one)
    un["Normal"][:33] = S.compress_sr11g11b10(_unit(_rng(131), 33) * [1, 1, 0] + [0, 0, 0.3])
    for k in range(33):                                                                                                          # x code == y code: inside the null space of (1, -1, 0)
        w = int(un["Normal"][k]); un["Normal"][k] = (w & ~(2047 << 11)) | ((w & 2047) << 11)
    rank1 = np.outer([0.5, -1.0, 2.0], [1.0, -1.0, 0.0])
    out.append(_case("j_rank1", "joints", un, [affine(rank1, (0.5, 0.5, 0.5))], tags=("nan_vector", "null_space_normal_33")))
    un = verts(66, 14, **one); un["Normal"][:17] = 0xFFFFFFFF; un["Normal"][17:33] = 0                                          # (1, 1, 1) and (-1, -1, -1): the null space
    rank2 = np.array([[1.0, -1.0, 0.0], [0.0, 1.0, -1.0], [1.0, 0.0, -1.0]])
    out.append(_case("j_rank2", "joints", un, [affine(rank2, (0.0, 0.25, 0.0))], tags=("nan_vector", "null_space_normal_33")))
    zr = rot_y(0.7) @ rot_x(0.3); zy = zr.copy(); zy[1] = 0.0; zz = zr.copy(); zz[2] = 0.0
    un = verts(129, 15, **two); un["JointIndices"][1::2] = (1, 0, 1, 0)
    out.append(_case("j_zero_row", "joints", un, [affine(zy, (0.25, 0.0, -0.5)), affine(zz, (0.0, 0.125, 0.0))], tags=("tie", "frame")))   # the component is +-0: u = 0.5, codes 1023.5 / 511.5
    out.append(_case("j_scale_1e20", "joints", verts(65, 16, **one), [affine(rot_y(0.2) * 1e20)], tags=("dot_overflow", "tie")))            # dot = Inf, 1 / Inf = 0: the vector is 0
    out.append(_case("j_scale_1e-30", "joints", verts(65, 17, **one), [affine(rot_y(0.2) * 1e-30)], tags=("inf_vector",)))                  # dot = 0, 1 / 0 = Inf
    nzj = affine(np.eye(3)); nzj[nzj == 0] = NZ
    out.append(_case("j_negative_zero", "joints", verts(65, 18, **one), [nzj]))
    nj = affine(rot_y(0.1)); nj[1, 1] = NAN
    out.append(_case("j_nan_entry", "joints", verts(65, 19, **one), [nj], tags=("nan_vector", "nan_position")))
    ij = affine(rot_y(0.1)); ij[0, 2] = INF
    out.append(_case("j_inf_entry", "joints", verts(65, 20, **one), [ij], tags=("nan_vector", "nan_position")))                 # dot = Inf: Inf * 0 = NaN in x, 0 elsewhere; the position's x is Inf or (z == 0) NaN
    out.append(_case("j_translation_flt_max", "joints", verts(65, 21, **one), [affine(rot_y(0.1), (FLT_MAX, -FLT_MAX, FLT_MAX))]))
    # ------------------------------------------------------------------------------------------------------------------ codes
    I2 = [affine(np.eye(3)), affine(rot_y(0.9) @ rot_x(0.4))]
    un = verts(66, 30, **two); un["JointIndices"][1::2] = (1, 0, 1, 0)
    words = np.uint32([0, 0xFFFFFFFF, MID_HI, MID_LO])
    un["Normal"][:32] = words[np.arange(32) % 4]; un["Tangent"][:32] = words[(np.arange(32) // 4) % 4]
    out.append(_case("c_extreme_and_mid_words", "codes", un, I2))
    un = verts(66, 31, **two); un["JointIndices"][1::2] = (1, 0, 1, 0)
    axes = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    un["Normal"][:60] = S.compress_sr11g11b10(axes[np.arange(60) % 6]); un["Tangent"][:60] = S.compress_sr11g11b10(axes[(np.arange(60) + 2) % 6])
    out.append(_case("c_axis_aligned", "codes", un, I2))
    un = verts(66, 32, **two); un["JointIndices"][1::2] = (1, 0, 1, 0)
    un["Tangent"][:33] = un["Normal"][:33]
    w = un["Normal"][33:].astype(np.uint32)
    un["Tangent"][33:] = (2047 - (w & 2047)) | ((2047 - ((w >> 11) & 2047)) << 11) | ((1023 - ((w >> 22) & 1023)) << 22)
    out.append(_case("c_parallel_normal_tangent", "codes", un, [affine(rot_y(0.9) @ np.diag([1.0, 3.0, 0.25])), affine(np.diag([2.0, -1.0, 0.5]))], tags=("parallel",)))
    out.append(_tie_down_case())
    # ------------------------------------------------------------------------------------------------------------------ indices
    J5 = np.stack([affine(rot_y(0.2 * k) @ rot_x(0.1 * k), (0.125 * k, 0.0, -0.25 * k)) for k in range(5)])
    out.append(_case("i_four_equal", "indices", verts(65, 40, indices=(3, 3, 3, 3)), J5))
    out.append(_case("i_last_joint_by_offset", "indices", verts(65, 41, indices=(2, 0, 1, 2)), J5, args=(0, PAD, 2, 65), tags=("reaches_last_joint",)))
    out.append(_case("i_offset_index_zero", "indices", verts(65, 42, indices=(0, 0, 0, 0), weights=(0.25, 0.25, 0.25, 0.25)), J5, args=(0, PAD, 4, 65), tags=("reaches_last_joint",)))
    # ------------------------------------------------------------------------------------------------------------------ ranges
    for n in (0, 1, 63, 64, 65, 129):
        out.append(_case(f"r_count_{n}", "ranges", verts(max(n, 1) + 1, 50 + n), G, args=(1, PAD + 2, 0, n), main=n + 7))
    out.append(_case("r_input_is_not_output", "ranges", verts(100, 60), G, args=(30, PAD + 3, 0, 65), main=75))
    out.append(_case("r_ends_at_both_tables", "ranges", verts(80, 61), G, args=(15, PAD + 5, 0, 65), main=70, tags=("ends_at_tables",)))
    out.append(_case("r_twice", "ranges", verts(70, 62), G, args=(2, PAD + 1, 0, 65), main=70, joints2=G[::-1].copy()))
    out.append(_case("r_whole_table", "ranges", verts(PAD + 60, 66), G, args=(0, 0, 0, PAD + 60), main=60, tags=("whole",)))         # the pad too: the whole vertex table is rewritten
    un = verts(70, 63); un["JointIndices"][0] = (9, 0, 0, 0); un["JointIndices"][66] = (0, 0, 0, 0xFFFFFFFF)                 # both neighbours of the range address no joint: still accepted
    out.append(_case("r_bad_neighbours", "ranges", un, G, args=(1, PAD, 0, 65), main=70, tags=("bad_neighbours",)))
    # a whole block of valid vertices BEHIND the range in both tables: a guard rounded up to the block of 64 would skin them too, without leaving any buffer
    out.append(_case("r_slack_behind_65", "ranges", verts(130, 64), G, args=(0, PAD, 0, 65), main=130, tags=("slack",)))
    out.append(_case("r_slack_behind_1", "ranges", verts(130, 65), G, args=(0, PAD, 0, 1), main=130, tags=("slack",)))
    # ------------------------------------------------------------------------------------------------------------------ refit geometries (finite positions by construction)
    keep = np.zeros((1, 3, 4), f32); keep[0, :, :3] = np.eye(3)
    out.append(_case("g_one_triangle", "refit", verts(3, 70, **one), [affine(rot_y(0.3), (0.5, 0.0, 0.0))], args=(0, PAD, 0, 3), main=3, geometry="one_triangle"))
    out.append(_case("g_fat_leaf", "refit", verts(24, 71, **one), [affine(rot_y(0.3) @ np.diag([1.0, 2.0, 0.5]))], args=(0, PAD, 0, 24), main=24, geometry="fat_leaf"))
    out.append(_case("g_collapse", "refit", verts(65, 72, **one), [affine(np.zeros((3, 3)), (0.25, -0.5, 0.125))], args=(0, PAD, 0, 65), main=65, tags=("zero_extent", "nan_vector")))
    # +0 / -0 planted on every axis.  Identity whose zero entries are -0 keeps the sign of a zero coordinate when the others are >= 0 ((1 * -0 + -0 * y) + -0 * z) + -0 = -0);
    # with zero entries +0 and translation -0 it does for coordinates <= 0.  All other coordinates on one side of zero: the zeros ARE the box faces, and every union meets a tie.
    for name, sign, zero in (("g_zeros_are_min", 1.0, NZ), ("g_zeros_are_max", -1.0, 0.0)):
        un = verts(66, 73 if sign > 0 else 74, **one)
        p = np.abs(un["Position"]) + f32(0.015625)
        zs = np.float32([0.0, NZ])
        for k in range(66):
            p[k, k % 3] = zs[(k // 3) % 2]; p[k, (k + 1) % 3] = zs[(k // 2) % 2] if k % 4 == 0 else p[k, (k + 1) % 3]
        un["Position"] = (p * f32(sign)).astype(f32)
        j = affine(np.eye(3)); j[j == 0] = zero; j[:, 3] = NZ
        out.append(_case(name, "refit", un, [j], args=(0, PAD, 0, 66), main=66, tags=("signed_zeros",)))
    un = verts(65, 75, **one); un["Position"] = (un["Position"] * f32(FLT_MAX / 8)).astype(f32)
    out.append(_case("g_flt_max_quarter", "refit", un, keep, args=(0, PAD, 0, 65), main=65, tags=("huge",)))
    un = verts(65, 76, **one); un["Position"] = (un["Position"] * f32(2.0 ** -140)).astype(f32)
    out.append(_case("g_subnormal", "refit", un, keep, args=(0, PAD, 0, 65), main=65, tags=("subnormal",)))
    # ------------------------------------------------------------------------------------------------------------------ refused (never launched)
    un = verts(65, 80); un["JointIndices"][64] = (0, 1, 0, 2); un["JointWeights"][64] = (0.5, 0.5, 0, 0)                         # the LAST vertex of the range, with weight 0 on the bad index
    out.append(_case("x_index_past_table", "refused", un, G, refused="joint"))
    out.append(_case("x_offset_past_table", "refused", verts(65, 81, indices=(0, 0, 0, 0)), G, args=(0, PAD, 2, 65), refused="joint"))
    un = verts(65, 82, indices=(0, 0, 0, 0)); un["JointIndices"][7, 1] = 1
    out.append(_case("x_offset_plus_index_wraps", "refused", un, G, args=(0, PAD, 0xFFFFFFFF, 65), refused="joint"))              # 2^32 - 1 + 1 wraps to joint 0 in 32 bits
    out.append(_case("x_input_range_past_table", "refused", verts(65, 83), G, args=(1, PAD, 0, 65), main=80, refused="range"))
    out.append(_case("x_output_range_past_table", "refused", verts(65, 84), G, args=(0, PAD + 16, 0, 65), main=80, refused="range"))
    out.append(_case("x_output_offset_wraps", "refused", verts(65, 85), G, args=(0, 0xFFFFFFF0, 0, 65), main=80, refused="range"))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FRAME_CASES = tuple(c["name"] for c in CASES if "frame" in c["tags"])


def rest_positions(n, seed=99):
    """rest positions of the skinned mesh (the BLAS topology is built from them; a refit only reads the skinned ones)"""
    return _dyadic(_rng(seed), (n, 3), span=1.5)


def geometry_indices(case):
    n, g = case["main"], case["geometry"]
    if g == "one_triangle":
        return np.uint32([[0, 1, 2]])
    if g == "fat_leaf":
        return np.arange(n, dtype=np.uint32).reshape(-1, 3)
    return np.stack([np.arange(n - 2), np.arange(1, n - 1), np.arange(2, n)], 1).astype(np.uint32)


def scene(case, builder, sky_color=(0.7, 0.8, 1.0)):
    """the scene a case is skinned in (module docstring): pad BLAS 0, skinned refittable BLAS 1"""
    n = case["main"]
    rng = _rng(7)
    pp, pi, pn, ptn = S.flat_shaded(S.soup_triangles(4, seed=5, extent=0.5, edge=0.4) + np.float32([0.0, -2.5, 0.0]))
    assert len(pp) == PAD
    if case["geometry"] == "fat_leaf":                                          # every triangle spans the same box: corners of one cube, the builder has nothing to split by
        corners = np.float32([[-1, -1, -1], [1, 1, 1], [1, -1, 1]])
        pos = np.tile(corners, (n // 3, 1)); pos[2::3, 1] = np.linspace(-1, 1, n // 3, dtype=np.float32)
    else:
        pos = rest_positions(n)
    main = S.MeshInput(pos, geometry_indices(case), S.make_material((0.8, 0.6, 0.5, 1.0)), _unit(rng, n), _unit(rng, n), uvs=_dyadic(rng, (n, 2), span=1.0))
    pad = S.MeshInput(pp, pi, S.make_material((0.5, 0.7, 0.9, 1.0), metallic=0.5, roughness=0.3), pn, ptn)
    return S.assemble([{"meshes": [pad]}, {"meshes": [main], "refittable": True}], builder, sky_color=sky_color)
