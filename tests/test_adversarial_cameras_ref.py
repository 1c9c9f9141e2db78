"""The adversarial cameras (tests/adversarial_cameras.py) are what they claim — shown on the CPU with the oracle alone (ref_primary_rays, ref_first_box_tests), no kernel
involved.  In particular the conditions that keep tests/test_gpu_adversarial_cameras.py from being vacuous: every silhouette / edge_on / near / lens / sky_faces case holds a
tile that can hit next to one that cannot (the sliver), a tile that cannot, and — sky_faces — a tile that sees two faces; every plain case holds a clearly empty tile."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adversarial_cameras as A  # noqa: E402

f32 = np.float32


@pytest.fixture(scope="module")
def scenes(native_builder):
    cache = {}

    def get(case):
        k = case.scene_key()
        if k not in cache:
            cache[k] = A.make_scene(case.scene, native_builder, sky=case.sky, **case.scene_kw)
        return cache[k]
    return get


def _contexts(case):
    """(member, local rows) of every context the case renders with"""
    n = case.rows[1] if case.rows and case.rows[0] == "members" else 1
    return [(m, A.local_rows(case, m)) for m in range(n)]


def _slivers(can):
    return int((can[:, 1:] != can[:, :-1]).sum() + (can[1:] != can[:-1]).sum())


@pytest.mark.parametrize("name", list(A.CASES))
def test_case_is_what_it_claims(oracle_mod, scenes, name):
    case = A.CASES[name]; sc = scenes(case)
    w, h = case.frame
    p = case.pf[0]; iv = p["InvView"].reshape(4, 4); eye = iv[3, :3]
    use_tlas = A.PLANS[A.plans_of(case)[0]][1]
    per = [(m, rows, A.truth(oracle_mod, case, sc, use_tlas, rows), A.clearly_empty(case, sc, use_tlas, rows)) for m, rows in _contexts(case)]
    can = np.concatenate([t.can_hit.ravel() for _, _, t, _ in per]); faces = np.concatenate([t.faces.ravel() for _, _, t, _ in per])
    slivers = sum(_slivers(t.can_hit) for _, _, t, _ in per); empty = sum(int(ce.sum()) for _, _, _, ce in per)
    print(f"{name}: {can.size} tiles, {int(can.sum())} can hit, {slivers} sliver edges, {int((faces & (faces - 1) != 0).sum())} tiles with two faces, {empty} clearly empty")
    # the doubled rule never calls a tile empty that a ray of the truth can hit from, or that sees two faces of a constant-per-face sky
    for _, _, t, ce in per:
        assert not (ce & t.can_hit).any(), name
        if sc.sky_faces is not None and sc.sky_faces.shape[1] == 1:
            assert ((t.faces[ce] & (t.faces[ce] - 1)) == 0).all(), name
    if case.cls in A.SLIVER_CLASSES:
        assert slivers > 0 and (~can).any(), f"{name}: no sliver"
        if case.cls == "sky_faces":
            assert (faces & (faces - 1) != 0).any(), f"{name}: no tile sees two faces"
    if case.plain:
        assert empty > 0, f"{name}: no clearly empty tile"
    # ---- per class
    root = sc.blas_nodes[sc.blas_descs[0]["NodeOffset"] + 1]; lo, hi = root["Min"], root["Max"]
    if case.cls == "silhouette_on_tile_edge":
        # the face z = -4 ends on the pixel columns 24 + dx and 40 + dx exactly (binary32 arithmetic on dyadic numbers)
        assert (eye == 0).all() and hi[2] == f32(-4.0)
        col = (np.float64([lo[0], hi[0]]) / 4.0 + 1.0) * 32.0
        want = {"exact": (24, 40), "plus_1px": (25, 41), "minus_1px": (23, 39), "plus_half": (24.5, 40.5), "minus_half": (23.5, 39.5)}.get(name[len("silhouette_"):])
        if want:
            assert tuple(col) == want
        else:
            assert col[0] == 24 and col[1] != 40 and abs(col[1] - 40) < 1e-5
    if case.cls == "apex":
        on = [(eye[a] == lo[a]) or (eye[a] == hi[a]) for a in range(3)]; inside = [(lo[a] <= eye[a] <= hi[a]) for a in range(3)]
        kind = name[len("apex_"):]
        if kind in ("inside", "on_face", "on_edge", "on_corner"):
            assert all(inside) and sum(on) == {"inside": 0, "on_face": 1, "on_edge": 2, "on_corner": 3}[kind]
        elif kind.startswith("behind"):
            assert eye[2] < lo[2] and not can.any() and (kind == "behind_on_axis") == (eye[0] == 0 and eye[1] == 0)
        else:
            assert lo[2] < eye[2] < hi[2] and not all(inside)
    if case.cls == "edge_on":
        assert lo[1] == hi[1] == 0.0 and abs(eye[1]) <= 1.5e-45 and (name.endswith("in_plane") == (eye[1] == 0.0))
    if case.cls == "far":
        d = float(np.linalg.norm(np.float64(eye) - (np.float64(lo) + hi) / 2))
        assert 2.0 / (2.0 * d / w) < 1.0 and d > 9e3                                  # the box is smaller than a pixel
        assert case.radius == 0.0 and 1e-4 * (d + 1.0) >= 1.0                          # ... and the margin is its 1e-4 * (D + 1) term alone, at least the box's half extent
        # ... and lies between pixel centres: no centre's ray (jitter 1/2) passes its box test, the box's centre projects off every pixel centre by more than its own size
        ctr = (np.float64(lo) + hi) / 2 - np.float64(eye); px = (ctr[0] / -ctr[2] + 1.0) * w / 2.0
        assert abs(px - np.floor(px) - 0.5) * (2.0 * d / w) > 2.0
    if case.cls == "fov":
        ip = p["InvProjection"]
        fovy = 2.0 * np.degrees(np.arctan(abs(float(ip[5]))))
        want = {"fov_1deg": 1.0, "fov_170deg": 170.0}.get(name, 90.0)
        assert abs(fovy - want) < 1e-3
        assert (ip[5] < 0) == (name == "fov_flip_y")
        assert ((ip[1] != 0) and (ip[4] != 0)) == (name == "fov_off_diagonal")
    if case.cls == "tiny":
        shape = per[0][2].can_hit.shape
        assert (w, h) in ((8, 8), (9, 7)) and shape == ((1, 1) if w == 8 else (1, 2))
        want = {"tiny_8x8_hit": [1], "tiny_8x8_empty": [0], "tiny_8x8_in_slack": [0], "tiny_9x7_whole_hits": [1, 0], "tiny_9x7_cut_hits": [0, 1]}[name]
        assert can.astype(int).tolist() == want
        if name == "tiny_8x8_in_slack":                                               # not reachable, yet inside the pixel of slack: the documented rule itself keeps it
            assert empty == 0 and not A.clearly_empty(case, sc, 0, factor=1.0).any()
    if name == "lens_sheared_near":
        ip = p["InvProjection"]
        assert ip[4] == -ip[5] and f32(case.radius) / f32(case.focal) <= f32(0.05)
        d = np.abs(np.float64([lo, hi]) - np.float64(eye)).max()
        assert d <= 0.1 * case.focal
        # it is the rim of the lens that reaches the box: with the lens points inside the unit circle only ... (the rule written with the radius itself called tiles empty that can hit)
        old = A.LENS_RIM
        try:
            A.LENS_RIM = 1.0
            assert (A.clearly_empty(case, sc, 0, factor=1.0) & per[0][2].can_hit).any()
        finally:
            A.LENS_RIM = old
        assert not (A.clearly_empty(case, sc, 0, factor=1.0) & per[0][2].can_hit).any()
    if name in ("sky_textured", "sky_none"):
        assert (sc.sky_faces is None) == (name == "sky_none") and (name == "sky_none" or sc.sky_faces.shape == (6, 2, 2, 4))
    if case.cls == "near":
        assert eye[0] - hi[0] == f32(2.0 ** -10) and lo[2] < eye[2] < hi[2]
    if case.cls == "lens":
        q = f32(case.radius) / f32(case.focal)
        if name in ("lens_at_gate", "lens_below_gate"):
            assert q <= f32(0.05) and (name == "lens_below_gate" or f32(A.ulps(case.radius, 1)) / f32(case.focal) > f32(0.05))
        if name == "lens_above_gate":
            assert q > f32(0.05) and f32(A.ulps(case.radius, -1)) / f32(case.focal) <= f32(0.05)
        if name == "lens_focal_at_gate":
            assert f32(case.focal) == f32(1e-3)
        if name == "lens_focal_above_gate":
            assert f32(case.focal) == np.nextafter(f32(1e-3), f32(1)) and q <= f32(0.05)
        if name.startswith("lens_focus"):
            z0, z1 = -float(hi[2]), -float(lo[2])
            assert {"in_front": case.focal < z0, "inside": z0 < case.focal < z1, "behind": case.focal > z1}[name[len("lens_focus_"):]]
    if case.cls == "apex_mismatch":
        d = np.abs(p["ViewPos"].view(np.int32).astype(np.int64) - eye.view(np.int32).astype(np.int64))
        assert (d > 0).all() and d.max() <= 4
    if case.cls == "bands":
        assert (w, h) in ((75, 37), (72, 40))                                        # a cut tile column and row; whole tiles only
        if case.rows[0] == "range":
            rows = per[0][1]
            assert rows[0] == 8 and len(rows) % 8 != 0
    if name == "sky_x_z_lens_aimed":
        # the tiles of columns 32-39 see two faces only through the lens: with radius 0 the same camera shows them one
        f1 = A.truth(oracle_mod, A.Case("no_lens", "sky_faces", pf=case.pf, focal=case.focal, radius=0.0), sc, 0).faces
        f2 = per[0][2].faces
        assert ((f1[:, 4] & (f1[:, 4] - 1)) == 0).all() and ((f2[:, 4] & (f2[:, 4] - 1)) != 0).all()
    if name in ("inst256", "inst257"):
        assert len(sc.blas_instances) == int(name[4:])
    if name == "tlas_leaf_root":
        assert (int(sc.tlas_nodes[0]["IsLeafAndChildOrInstanceId"]) >> 31) == 1 and can.all()
    if name.startswith("sky_") and name.split("_")[1] in ("x", "diag", "z") and "lens" not in name:
        # the centre of the frame looks exactly along the stated direction: components of equal magnitude
        v = -iv[2, :3]; nz = np.abs(v[v != 0])
        assert (nz == nz[0]).all()


def test_the_inst_scene_holds_the_stated_matrices(native_builder):
    sc = A.make_scene("inst", native_builder)
    m = sc.mesh_transforms["Model"].astype(np.float64); inv = sc.mesh_transforms["InvModel"].astype(np.float64)
    assert len(sc.blas_instances) == 9
    lin = m[:, :, :3]
    det = np.linalg.det(lin)
    assert (det < 0).sum() == 1                                                       # the mirror
    exact = [k for k in range(9) if set(np.unique(np.abs(lin[k]))) <= {0.0, 1.0}]
    assert len(exact) >= 6                                                            # identity, quarter turns, the mirror
    s = np.linalg.svd(lin, compute_uv=False)
    assert (s[:, 0] / s[:, 2] > 1e5).sum() == 1                                       # the needle: 1000 against 1/1000
    needle = int(np.argmax(s[:, 0] / s[:, 2]))
    # its InvModel is a rounded inverse: Model * InvModel differs from the identity — the classifier places boxes with Model, the rays are culled with InvModel
    prod = lin[needle] @ inv[needle][:, :3]
    assert np.abs(prod - np.eye(3)).max() > 0
    assert any(abs(lin[k][0, 1]) == 0.5 or abs(lin[k][1, 0]) == 0.5 for k in range(9))  # the shear


def test_the_lens_points_lie_on_the_rim_of_the_sampler():
    """Sampling.glsl:98-114: `point * 2 - 1` of a point of [0, 1)^2 with |point| <= 1 — the centre first, then 8 points of that set's boundary, (-1, -1) among them"""
    pnt = (A.LENS.astype(np.float64) + 1.0) / 2.0
    assert len(A.LENS) == 9 and (A.LENS[0] == 0).all() and (A.LENS[1] == -1).all()
    assert ((pnt >= 0) & (pnt < 1)).all() and ((pnt ** 2).sum(1) <= 1 + 1e-7).all()
    rim = (pnt[1:] == 0).any(1) | (np.abs((pnt[1:] ** 2).sum(1) - 1) < 1e-6) | (pnt[1:] >= 1 - 1e-7).any(1)
    assert rim.all()
    j = A.JITTERS
    assert len(j) == 81 and j.min() == 0 and j.max() == np.nextafter(f32(1), f32(0))
