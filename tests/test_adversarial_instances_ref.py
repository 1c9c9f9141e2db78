"""The adversarial instance sets (tests/adversarial_instances.py) are what they claim, shown on the CPU from a numpy census of the leaf boxes, and the product's host builder
(idkbvhBuildTlas, csrc/bvh_builder.cpp) gives the oracle's node array on every one of them, byte for byte, at every radius of the case."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adversarial_instances as A  # noqa: E402


@pytest.fixture(scope="module")
def built(native_builder, oracle_builder):
    """per case: the scene, the oracle's leaf bounds and the oracle's node array per radius — computed once, shared, never written to"""
    cache = {}

    def get(name):
        if name not in cache:
            case = A.CASES[name]
            sc = case.factory(native_builder)
            bounds = A.bounds_of(sc, oracle_builder)
            area = A.finite_union(bounds)
            cache[name] = (sc, bounds, {r: oracle_builder.build_tlas(bounds, r) for r in case.radii}, area)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(A.CASES))
def test_cases_meet_the_condition_and_the_census_restates_the_oracle(built, native_builder, name):
    """finite union area; the numpy restatement of Box.Transformed gives the oracle's leaf bounds bit for bit (signs of zero included), so the census speaks about the boxes
    the builders see; the product's Box.Transformed gives them too"""
    sc, bounds, _, area = built(name)
    assert np.isfinite(sc.mesh_transforms["Model"]).all() and np.isfinite(sc.blas_nodes["Min"]).all() and np.isfinite(sc.blas_nodes["Max"]).all()
    assert A.leaf_boxes(sc).view(np.uint32).tolist() == bounds.view(np.uint32).tolist()
    assert A.bounds_of(sc, native_builder).tobytes() == bounds.tobytes()
    assert len(sc.blas_descs) <= 6 and sc.blas_descs["TriangleCount"].max() <= 8      # (tiny BLASes: 1-4 triangles, PreSplit may cut one)


@pytest.mark.parametrize("name", list(A.CASES))
def test_host_builder_equals_the_oracle(built, native_builder, name):
    sc, bounds, want, _ = built(name)
    for r in A.CASES[name].radii:
        got = native_builder.build_tlas(bounds, r)
        assert got.tobytes() == want[r].tobytes(), f"{name} radius {r}: {A.first_difference(got, want[r])}"


def _reversed_union_differs(bounds, root, axis, side):
    """the oracle's root holds a zero on (side, axis) whose sign is not the sign a union of the same leaves in REVERSED instance order gives (minps rule, numpy)"""
    rev = A.union_in_order(bounds, range(len(bounds) - 1, -1, -1))
    k = axis + (3 if side == "Max" else 0)
    r = np.float32(root[side][axis])
    return r == 0 and rev[k] == 0 and bool(np.signbit(r)) != bool(np.signbit(rev[k]))


@pytest.mark.parametrize("name", list(A.CASES))
def test_every_class_reaches_what_it_names(built, name):
    case = A.CASES[name]
    sc, bounds, want, area = built(name)
    n = len(bounds)
    for r in case.radii:
        c = A.census(sc, r)
        print(f"{name} radius {r}: {c} union_half_area {area:.6g}")
        assert c["n"] == n
        if case.cls == "same_key":
            assert c["shared_keys"] > 0
            if case.claims.get("all_identical"):
                assert c["shared_keys"] == n
        if case.cls == "same_area":
            assert (c["tied_searches"] > 0) == (r >= case.claims["ties_from"])
        if case.cls == "flat":
            assert c["zero_extent_axes"] == case.claims["zero_axes"]
            # (all centres at one point: every component is 0 or 512, no centre can be the maximum of an axis with extent)
            assert (c["keys_with_1023"] > 0) == case.claims["at_max"]
        if case.cls == "signed_zero":
            assert c["zeros_pos"] > 0 and c["zeros_neg"] > 0
            assert _reversed_union_differs(bounds, want[r][0], case.claims["axis"], case.claims["side"]), (want[r][0], A.union_in_order(bounds, range(n - 1, -1, -1)))
        if case.cls in ("counts", "radius") and n >= 3:
            d = A.leaf_depths(want[r])
            assert len(d) == n and d.min() != d.max(), f"{name} radius {r}: a perfectly balanced tree: no round left a node unmerged"
    if case.cls == "flat":
        assert any(A.CASES[k].claims["at_max"] for k in A.CASES if A.CASES[k].cls == "flat")


@pytest.mark.parametrize("name", [k for k in A.CASES if A.CASES[k].cls == "transforms"])
def test_transformed_boxes_within_one_ulp_of_binary64(built, name):
    """Box.Transformed of the oracle against the 8 corners evaluated in binary64 from the same binary32 matrix and root box: within 1 ulp of binary32 per coordinate.
    Why 1 ulp holds for THESE scenes: a coordinate is ((a + b) + c) + t.  Under the scales, the shear and the quarter turns every product and partial sum is a small dyadic
    number, exact; only the last sum rounds (half an ulp).  Under the inexact turns the corner lies within 4.9 of the BLAS origin: |a|, |b|, |c| <= 4 (three rounded products,
    2^-23 each), two partial sums below 8 (2^-22 each), together 0.875 * 2^-21; t >= 16 keeps the result above 11, where an ulp is at least 2^-20, so what came before the last
    sum is below 0.44 ulp and the last sum adds half an ulp.  At the far translations (ulp 2^-3) everything before the last sum vanishes against it.
    Mirrored instances (negative determinant) must still give min <= max on every axis."""
    sc, bounds, _, _ = built(name)
    inst = sc.blas_instances
    root = sc.blas_nodes[sc.blas_descs[inst["BlasId"]]["NodeOffset"] + 1]
    M = sc.mesh_transforms["Model"][inst["MeshTransformId"]].astype(np.float64)
    corners = np.array([[[(root["Max"] if (c >> k) & 1 else root["Min"])[i, k] for k in range(3)] for c in range(8)] for i in range(len(inst))], np.float64)   # (n, 8, 3)
    w = np.einsum("nkj,ncj->nck", M[:, :, :3], corners) + M[:, None, :, 3]
    exact = np.concatenate([w.min(1), w.max(1)], 1)
    err = np.abs(bounds.astype(np.float64) - exact); ulp = np.spacing(np.abs(bounds)).astype(np.float64)
    names = A.transform_names()
    worst = np.unravel_index(np.argmax(err / ulp), err.shape)
    print(f"{name}: worst {err[worst] / ulp[worst]:.3f} ulp at instance {worst[0]} ({names[worst[0]]}) coordinate {worst[1]}")
    assert (err <= ulp).all(), [(names[i], int(k), float(err[i, k] / ulp[i, k])) for i, k in np.argwhere(err > ulp)]
    assert (bounds[:, :3] <= bounds[:, 3:]).all()
    dets = np.linalg.det(M[:, :, :3])
    for i, nm in enumerate(names):
        assert (dets[i] < 0) == (nm in A.MIRRORED), (nm, dets[i])
    assert abs(dets[names.index("zero_y")]) == 0 and (bounds[names.index("zero_y"), 1] == bounds[names.index("zero_y"), 4])


def test_the_case_list_covers_the_named_sizes_and_radii():
    C = A.CASES
    assert {C[k].cls for k in C} == set(A.CLASSES)
    assert [len(C[f"count_{n}"].radii) for n in A.COUNTS] == [1] * 14 and A.COUNTS == (1, 2, 3, 4, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000)
    assert C["radius_n40"].radii == (1, 2, 3, 15, 39, 40, 4096) and C["radius_n1025"].radii == (1, 2, 3, 15, 1024, 1025, 4096)
    for k in ("lattice_16", "lattice_8x8", "lattice_4x4x4"):
        assert C[k].radii[:3] == (1, 2, 15) and C[k].radii[3] >= 16
    for cls in A.CLASSES:
        assert sum(C[k].render for k in C if C[k].cls == cls) == 1, cls
