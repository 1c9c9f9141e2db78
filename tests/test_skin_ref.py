"""tests/skin_ref.py (what idkptSkin is held to) against the reference's own Skinning shader run on llvmpipe — the committed fixtures — and against hand-worked
answers; tests/adversarial_skeletons.py against itself: every case is the edge it claims to be.  CPU only."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import skin_ref as R  # noqa: E402
import adversarial_skeletons as A  # noqa: E402

f32 = np.float32


def test_restatement_equals_the_reference_shader_on_the_update_fixture(native_builder):
    """Skinning/compute.glsl on llvmpipe (tests/golden/glref/updates.npz): positions, previous positions, and ALL 590 re-compressed normals and 590 tangents word for word."""
    sys.path.insert(0, os.path.join(ROOT, "oracle", "glref"))
    import make_vectors as mv
    fx = np.load(os.path.join(HERE, "golden", "glref", "updates.npz"))
    sc, moved, un, joints, sk = mv.update_inputs(native_builder)
    pos, prev, verts = R.skin(un, joints, moved, sc.vertices, sk["input_offset"], sk["output_offset"], sk["joint_offset"], sk["count"])
    lo, hi = sk["output_offset"], sk["output_offset"] + sk["count"]
    assert pos[lo:hi].tobytes() == fx["skin_positions"].tobytes()
    assert prev[lo:hi].tobytes() == fx["skin_prev_positions"].tobytes() and not prev[:lo].any() and not prev[hi:].any()
    assert pos[:lo].tobytes() == moved[:lo].tobytes() and pos[hi:].tobytes() == moved[hi:].tobytes()
    assert (verts["Normal"][lo:hi] == fx["skin_normals"]).all() and (verts["Tangent"][lo:hi] == fx["skin_tangents"]).all() and hi - lo == 590
    out = np.ones(len(verts), bool); out[lo:hi] = False
    assert verts[out].tobytes() == sc.vertices[out].tobytes() and verts["TexCoord"].tobytes() == sc.vertices["TexCoord"].tobytes()


def test_restatement_equals_the_reference_shader_on_the_1m_samples(native_builder):
    """The sampled normals / tangents of the 3 M-vertex skinning fixture (tests/golden/glref_full/updates_1m.npz, every 1021st vertex: 2939 of each).  Measured share of equal
    words: 1.0 for both (profiles/skin_adversarial.md) — so equality is asserted, not the >= 98 % tests/test_gpu_glref_full.py holds the device to."""
    from test_glref_full import _mfv
    fx = np.load(os.path.join(HERE, "golden", "glref_full", "updates_1m.npz"))
    sc, moved, un, joints = _mfv().full_update_inputs(native_builder)
    st = R.intermediates(un[::1021], joints, 0)
    for field, key in (("Normal", "skin_normals_sample"), ("Tangent", "skin_tangents_sample")):
        same = st[field]["word"] == fx[key]
        print(field, "share of equal words", same.mean(), "of", len(same))
        assert len(same) == 2939 and same.all(), (field, same.mean())
    assert st["position"].tobytes() == fx["skin_positions_sample"].tobytes()


def test_compression_known_answers():
    """Worked by hand.  u = v / 2 + 1 / 2; code = rint(u * 2047) (z: 1023), ties to even; word = z << 22 | y << 11 | x."""
    # v = 0: u = 0.5, 0.5 * 2047 = 1023.5 -> 1024 (even), 0.5 * 1023 = 511.5 -> 512 (even): both tie codes
    assert int(R.compress(f32([[0.0, 0.0, 0.0]]))[0]) == 1024 | (1024 << 11) | (512 << 22) == A.MID_HI
    assert int(R.compress(f32([[-0.0, -0.0, -0.0]]))[0]) == A.MID_HI                      # -0 * 0.5 + 0.5 is the same 0.5
    # (a tie whose even neighbour is BELOW, e.g. 1022.5, needs a product that ROUNDS to it: the case j_tie_to_the_even_code_below finds such inputs; here the rounding itself)
    codes, scaled = R.compress_codes(f32([[0.0, 0.0, 0.0]]))
    assert scaled.tolist() == [[1023.5, 1023.5, 511.5]] and codes.tolist() == [[1024.0, 1024.0, 512.0]]
    assert np.rint(f32(1022.5)) == 1022 and np.rint(f32(510.5)) == 510 and np.floor(f32(1022.5) + f32(0.5)) == 1023    # ties to even is NOT floor(x + 0.5)
    # v = (1, 1, 1): u = 1, codes 2047, 2047, 1023: every bit set
    assert int(R.compress(f32([[1.0, 1.0, 1.0]]))[0]) == 0xFFFFFFFF
    assert int(R.compress(f32([[-1.0, -1.0, -1.0]]))[0]) == 0
    # a mirrored normal: (1, 0, 0) under diag(-1, 1, 1) is (-1, 0, 0): codes 0, 1024, 512
    un = A.verts(1, 0, indices=(0, 0, 0, 0), weights=(1, 0, 0, 0)); un["Normal"] = 2047 | (1024 << 11) | (512 << 22)       # decodes to (1, 1 / 2047, 1 / 1023)
    st = R.intermediates(un, A.affine(np.diag([-1.0, 1.0, 1.0]))[None], 0)
    assert st["Normal"]["decoded"][0].tolist() == [1.0, float(f32(1024) / f32(2047) * f32(2) - f32(1)), float(f32(512) / f32(1023) * f32(2) - f32(1))]
    assert int(st["Normal"]["word"][0]) == 0 | (1024 << 11) | (512 << 22)                 # x flips to code 0; y, z (tiny, positive) stay on the codes above the middle
    # decode . encode is the identity on every code of every field
    allx = np.arange(2048, dtype=np.uint32); w = allx | (allx << np.uint32(11)) | ((allx & np.uint32(1023)) << np.uint32(22))
    assert (R.compress(R.decompress(w)) == w).all()


def test_compression_rule_for_values_no_field_holds():
    """include/idkpt.h, idkptSkin: clamp each field to its own range before the conversion, NaN acts as 0.  No field may spill into its neighbour."""
    nan, inf = float("nan"), float("inf")
    assert int(R.compress(f32([[nan, nan, nan]]))[0]) == 0
    assert int(R.compress(f32([[inf, inf, inf]]))[0]) == 0xFFFFFFFF
    assert int(R.compress(f32([[-inf, -inf, -inf]]))[0]) == 0
    assert int(R.compress(f32([[inf, nan, -inf]]))[0]) == 2047
    assert int(R.compress(f32([[nan, inf, 0.0]]))[0]) == (2047 << 11) | (512 << 22)
    assert int(R.compress(f32([[-inf, 0.0, inf]]))[0]) == (1024 << 11) | (1023 << 22)
    assert int(R.compress(f32([[3.0, -3.0, 1e30]]))[0]) == 2047 | (1023 << 22)           # finite but beyond [-1, 1]: clamped the same way


def test_equality_helpers():
    a = f32([1.0, float("nan"), -0.0]); b = a.copy(); b.view(np.uint32)[1] = 0xFFC00001
    assert R.same_positions(a, b) and a.tobytes() != b.tobytes()
    assert not R.same_positions(f32([0.0]), f32([-0.0])) and not R.same_positions(f32([float("nan")]), f32([float("inf")])) and not R.same_positions(a, a[:2])
    v = np.zeros(2, A.T.GpuVertex); w = v.copy(); w["Normal"][1] = 1
    assert R.same_vertices(v, v.copy()) and not R.same_vertices(v, w)


def test_table_has_every_class_and_small_cases():
    assert {c["cls"] for c in A.CASES} == set(A.CLASSES)
    need = {"weights": 8, "joints": 13, "codes": 3, "indices": 3, "ranges": 13, "refit": 7, "refused": 6}
    for cls, n in need.items():
        assert sum(c["cls"] == cls for c in A.CASES) >= n, cls
    assert all(len(c["un"]) <= 130 and c["main"] <= 302 for c in A.CASES)
    assert sorted(c["args"][3] for c in A.CASES if c["name"].startswith("r_count_")) == [0, 1, 63, 64, 65, 129]
    assert set(A.FRAME_CASES) == {"j_mirror", "j_nonuniform", "j_zero_row"}


@pytest.mark.parametrize("case", A.CASES, ids=[c["name"] for c in A.CASES])
def test_every_case_is_the_edge_it_claims(case, native_builder):
    sc = A.scene(case, native_builder)
    i, o, j, n = case["args"]
    tags = case["tags"]
    assert len(sc.vertices) == A.PAD + case["main"] and len(sc.blas_descs) == 2 and sc.blas_descs[1]["IsRefittable"] == 1
    d = sc.blas_descs[1]
    assert d["NodeOffset"] > 0 and d["TriangleOffset"] > 0 and d["TriangleCount"] <= 300
    why = R.refusal(case["un"], len(case["joints"]), len(sc.vertices), i, o, j, n)
    assert why == case["refused"]
    if case["refused"]:
        assert case["cls"] == "refused"
        if case["name"] == "x_offset_plus_index_wraps":
            assert (j + int(case["un"]["JointIndices"].max())) % 2 ** 32 < len(case["joints"])      # in 32 bits the sum lands INSIDE the table
        if case["name"] == "x_output_offset_wraps":
            assert (o + n) % 2 ** 32 <= len(sc.vertices)
        if case["name"] == "x_index_past_table":                                                       # one vertex, the last of the range, and the bad index has weight 0
            bad = (case["un"]["JointIndices"] >= len(case["joints"]))
            assert bad.sum() == 1 and bad[i + n - 1].any() and case["un"]["JointWeights"][bad][0] == 0
        return
    assert case["cls"] != "refused"
    if n == 0:
        return
    st = R.intermediates(case["un"][i:i + n], case["joints"], j)
    vec = np.concatenate([st["Normal"]["normalized"], st["Tangent"]["normalized"]])
    scaled = np.concatenate([st["Normal"]["scaled"], st["Tangent"]["scaled"]])
    dots = np.concatenate([st["Normal"]["dot"], st["Tangent"]["dot"]])
    assert ("nan_vector" in tags) == bool(np.isnan(vec).any()), "NaN reaches the compression exactly where the case says"
    assert ("inf_vector" in tags) == bool(np.isinf(vec).any())
    assert ("nan_position" in tags) == bool(np.isnan(st["position"]).any())
    assert ("dot_overflow" in tags) == bool(np.isinf(dots).any())
    with np.errstate(invalid="ignore"):
        ties = (scaled - np.floor(scaled)) == 0.5
    if "tie" in tags:                                                                                   # (other cases may meet a tie by chance: a component below 2^-25 also gives u == 0.5)
        assert ties[:, :2].any() and ties[:, 2].any() and set(scaled[ties].tolist()) == {1023.5, 511.5}
    if "tie_down" in tags:                                                                              # k + 0.5 with k even, in both field widths: rint and floor(x + 0.5) part
        sn = st["Normal"]["scaled"]
        down = ((sn - np.floor(sn)) == 0.5) & (np.floor(sn) % 2 == 0)
        assert down[:, 1].sum() >= 8 and down[:, 2].sum() >= 8 and (st["Normal"]["codes"][down] == np.floor(sn[down])).all() and (np.floor(sn[down] + f32(0.5)) == st["Normal"]["codes"][down] + 1).all()
    if "whole" in tags:
        assert o == 0 and n == len(sc.vertices)
    if "zero_matrix" in tags:
        assert not st["M"].any()
    if "null_space_normal_33" in tags:                                                                  # inside the null space: exactly 0 -> NaN; outside: finite
        assert np.isnan(st["Normal"]["normalized"][:33]).all() and (st["Normal"]["dot"][:33] == 0).all() and np.isfinite(st["Normal"]["normalized"][33:]).all()
    if "reaches_last_joint" in tags:
        assert j > 0 and j + int(case["un"]["JointIndices"][i:i + n].max()) == len(case["joints"]) - 1
    if "ends_at_tables" in tags:
        assert i + n == len(case["un"]) and o + n == len(sc.vertices) and i != o
    if "bad_neighbours" in tags:
        assert case["un"]["JointIndices"][i - 1].max() >= len(case["joints"]) and case["un"]["JointIndices"][i + n].max() >= len(case["joints"])
    if "slack" in tags:
        up = (n + 63) // 64 * 64
        assert up > n and i + up <= len(case["un"]) and o + up <= len(sc.vertices) and j + int(case["un"]["JointIndices"].max()) < len(case["joints"])
    if "parallel" in tags:
        dn, dt = st["Normal"]["decoded"], st["Tangent"]["decoded"]
        assert (dn[:33] == dt[:33]).all() and np.abs(dn[33:] + dt[33:]).max() < 2e-7
    if case["name"] == "c_extreme_and_mid_words":
        assert {0, 0xFFFFFFFF, A.MID_HI, A.MID_LO} <= set(case["un"]["Normal"].tolist()) and {0, 0xFFFFFFFF, A.MID_HI, A.MID_LO} <= set(case["un"]["Tangent"].tolist())
    pos, prev, verts = R.skin(case["un"], case["joints"], sc.vertex_positions, sc.vertices, i, o, j, n)
    if case["cls"] == "refit" or "frame" in tags:
        assert np.isfinite(pos).all()
    nodes = sc.blas_nodes[d["NodeOffset"]: d["NodeOffset"] + d["NodeCount"]]
    if case["geometry"] == "one_triangle":
        assert d["NodeCount"] == 4 and nodes["TriCount"].tolist() == [0, 0, 1, 1] and nodes["TriStartOrChild"][1] == 2   # the one leaf duplicated into nodes 2 and 3 under the root
        assert (nodes["Min"][2:] == nodes["Min"][1]).all() and (nodes["Max"][2:] == nodes["Max"][1]).all()
    elif n >= 8:
        assert nodes["TriCount"].max() >= 2                                                             # a leaf with several triangles
    p = pos[o:o + n]
    if "zero_extent" in tags:
        assert (p == p[0]).all()
    if "signed_zeros" in tags:
        edge = p.min(0) if case["name"].endswith("min") else p.max(0)
        assert (edge == 0).all()
        for k in range(3):
            z = p[:, k] == 0
            assert (np.signbit(p[:, k]) & z).sum() >= 5 and (~np.signbit(p[:, k]) & z).sum() >= 5, "both zeros on every axis, and they are the box's face"
    if "huge" in tags:
        assert np.abs(p).max() >= A.FLT_MAX / 4 and np.isfinite(p).all()
    if "subnormal" in tags:
        assert 0 < np.abs(p[p != 0]).max() < np.finfo(f32).tiny
    if case["joints2"] is not None:
        pos2, prev2, _ = R.skin(case["un"], case["joints2"], pos, verts, i, o, j, n, prev_positions=prev)
        assert prev2[o:o + n].tobytes() == pos[o:o + n].tobytes() != prev[o:o + n].tobytes() and pos2.tobytes() != pos.tobytes()


def test_refit_oracle_pins_the_second_operand_on_zero_ties(oracle_builder, native_builder):
    """Box.GrowToFit is minps / maxps: equal operands give the SECOND.  On the planted zeros the oracle's (and the host builder's) refit therefore stores zeros of BOTH signs in box
    faces — an order-independent minimum (-0 < +0) would store only one."""
    for name in ("g_zeros_are_min", "g_zeros_are_max"):
        case = A.BY_NAME[name]
        sc = A.scene(case, native_builder)
        pos, _, _ = R.skin(case["un"], case["joints"], sc.vertex_positions, sc.vertices, *case["args"])
        d = sc.blas_descs[1]
        sl = slice(d["NodeOffset"], d["NodeOffset"] + d["NodeCount"])
        tris = sc.blas_triangles[d["TriangleOffset"]: d["TriangleOffset"] + d["TriangleCount"]]
        want = oracle_builder.refit(sc.blas_nodes[sl], pos, tris)
        assert native_builder.refit(sc.blas_nodes[sl], pos, tris).tobytes() == want.tobytes()
        face = want["Min" if name.endswith("min") else "Max"][1:]
        z = face == 0
        assert (np.signbit(face) & z).any() and (~np.signbit(face) & z).any()
