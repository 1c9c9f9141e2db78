"""CPU proof that the adversarial surface classes (tests/adversarial_surfaces.py) are what they claim.  Every (scene, settings) pair of tests/test_gpu_adversarial_surfaces.py is
rendered in the oracle with its branch record on (OraclePathTracer.set_branch_record: one word of flags per shaded hit + the mesh it hit), and the classes are asked for
witnesses: the branch a swatch was built for must show in at least FLOOR shaded hits at each frame size of the GPU test, and a branch a swatch was built to avoid must never show
on it.  The floor is met by the SUM over the cases that render the swatch at that frame size (three cameras, three forms), not by every case alone: a single swatch covers about
15 pixels of the ragged frame.  The floor is a literal; a swatch that falls short is to be enlarged or moved.  The planted frames (draws equal to the chance) hold one witness
each by construction."""
import os
import sys
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import adversarial_surfaces as A  # noqa: E402
import adversarial_rays as AR  # noqa: E402

FLOOR = 16
FLT_MIN = np.float32(1.17549435e-38)


def _finite(o):
    r = o.rays()
    arrays = [o.image(0), o.image(1), o.image(2), o.primary_hits()[0], o.primary_hits()[2]] + [r[f] for f in r.dtype.names]
    return all(np.isfinite(a).all() for a in arrays)


@pytest.fixture(scope="module")
def records(native_builder, oracle_mod):
    """{(case id, frame): (scene, flags, what)} of the default settings of every case, and the finiteness of every (case, settings) pair — rendered once"""
    rec, finite = {}, {}
    settings = {}
    for _, _, ov, frames, _ in A.VARIANTS:
        settings[A.settings_key({}, ov, frames)] = (ov, frames)
    for cid, cls, form, use_tlas, cam, base in A.cases():
        sc = A.cached_room(form, native_builder)
        for (w, h) in A.FRAMES:
            pf = A.case_camera(sc, cam, w, h)
            for key, (ov, frames) in settings.items():
                d = dict(base, UseTlas=use_tlas); d.update(ov)
                o, r = A.render_oracle(oracle_mod, sc, pf, w, h, d, frames, record=not ov and frames == 1)
                finite[(cid, (w, h), key)] = _finite(o)
                if r is not None:
                    rec[(cid, (w, h))] = (sc, r[0].copy(), r[1].copy(), o.image(0), cls)
                o.close()
    return rec, finite


def _count(records, frame, names, need=(), avoid=(), classes=None, bounce=None, xform=None):
    """shaded hits, at one frame size over all cases, on swatches called `names` (or their copies `name_b` on wall B) whose flags have all of `need` and none of `avoid`"""
    B = _count.B
    total = 0
    for (cid, fr), (sc, fl, what, _, _) in records.items():
        if fr != frame:
            continue
        f = fl if bounce is None else fl[:, bounce: bounce + 1]; wh = what if bounce is None else what[:, bounce: bounce + 1]
        mesh = (wh & 0xFFFF).astype(np.int64) - 1
        is_tri = (wh != 0) & ((wh >> 31) == 0)
        sel = (f & B["shaded"]) != 0
        if names is not None:
            ids = [k for k, n in enumerate(sc.swatch_name) if n in names or (n.endswith("_b") and n[:-2] in names)]
            sel &= is_tri & np.isin(mesh, ids)
        if classes is not None:
            ids = [k for k, c in enumerate(sc.swatch_class) if c in classes]
            sel &= is_tri & np.isin(mesh, ids)
        if xform is not None:
            sel &= is_tri & (((wh >> 16) & 0x7FFF) == xform)
        for n in need:
            sel &= (f & B[n]) != 0
        for n in avoid:
            sel &= (f & B[n]) == 0
        total += int(sel.sum())
    return total


CLAMPS = ("metallic_lo", "metallic_hi", "roughness_lo", "roughness_hi", "transmission_lo", "transmission_hi", "ior_lo", "absorbance_lo")
# (swatch, flags that must show together in >= FLOOR hits, flags that must NEVER show on the swatch)
CLAIMS = [
    # alpha_edges
    ("cutoff_0", ("shaded",), ("alpha_skip", "blend")), ("alpha_equals_cutoff", ("shaded",), ("alpha_skip",)), ("alpha_ulp_below_cutoff", ("alpha_skip",), ("bsdf0", "bsdf1", "bsdf2")),
    ("cutoff_1_alpha_1", ("shaded",), ("alpha_skip",)), ("blend_alpha_0", ("blend", "alpha_skip"), ()), ("blend_alpha_1", ("blend",), ("alpha_skip",)),
    ("cutoff_above_2", ("alpha_skip",), ("blend", "bsdf0", "bsdf1", "bsdf2")), ("stack_base", ("shaded",), ("alpha_skip",)),
    # chance_edges
    ("metallic_1", ("bsdf1",), ("bsdf0", "bsdf2")), ("transmission_1", ("bsdf2",), ("bsdf0",)), ("both_1", ("bsdf1",), ("bsdf0", "bsdf2")), ("both_0", ("bsdf0",), ("bsdf2",)),
    ("ior_equals_previous", ("bsdf0",), ("bsdf2",)), ("ior_1_both_sides", ("bsdf2", "inside"), ()), ("ior_1e6", ("bsdf1",), ()), ("ior_bias_below_1", ("ior_lo",), ()),
    # clamp_edges
    ("SpecularBias_plus_10", ("metallic_hi",), ("metallic_lo",)), ("SpecularBias_minus_10", ("metallic_lo",), ("metallic_hi",)), ("RoughnessBias_plus_10", ("roughness_hi",), ("roughness_lo",)),
    ("RoughnessBias_minus_10", ("roughness_lo",), ("roughness_hi",)), ("TransmissionBias_plus_10", ("transmission_hi",), ("transmission_lo",)),
    ("TransmissionBias_minus_10", ("transmission_lo",), ("transmission_hi",)), ("IORBias_plus_10", ("shaded",), ("ior_lo",)), ("IORBias_minus_10", ("ior_lo",), ()),
    ("lands_on_1", ("on_bound",), CLAMPS), ("lands_on_0", ("on_bound",), CLAMPS), ("negative_zero_biases", ("shaded",), CLAMPS + ("on_bound",)),
    ("absorbance_below_0", ("absorbance_lo", "absorb"), ()), ("AbsorbanceBias_plus_10", ("absorb",), ("absorbance_lo",)), ("AbsorbanceBias_minus_10", ("absorbance_lo", "absorb"), ("exp_underflow",)), ("emissive_bias", ("shaded",), CLAMPS),
    # roughness_edges
    ("diffuse_r0", ("bsdf0",), ()), ("diffuse_r1", ("bsdf0",), ()), ("specular_r0", ("bsdf1",), ("bsdf0", "bsdf2")), ("specular_r1", ("bsdf1",), ("bsdf0", "bsdf2")),
    ("transmissive_r0", ("bsdf2",), ("bsdf0",)), ("transmissive_r1", ("bsdf2",), ("bsdf0",)),
    # volume_edges
    ("absorbance_0", ("absorb",), ("exp_underflow", "throughput_zero")), ("absorbance_straddles_87", ("absorb", "exp_underflow"), ()), ("absorbance_1e30", ("exp_underflow", "throughput_zero"), ()),
    ("tir_ior_1_5", ("tir",), ()), ("tir_ior_2_4", ("tir",), ()), ("thin_walled", ("thin",), ("absorb", "tir")), ("thin_walled_tint_0", ("thin", "inside"), ("absorb",)),
    ("tint_0", ("bsdf2", "inside"), ()), ("tint_1", ("bsdf2", "inside"), ()),
    # frame_edges
    ("normal_map_strength_0", ("shaded",), ()), ("normal_map_strength_1", ("shaded",), ()), ("normal_map_strength_2", ("shaded",), ()), ("normal_map_strength_-1", ("shaded",), ()),
    ("normal_texel_half", ("shaded",), ()), ("normal_texel_one", ("shaded",), ()), ("normal_texel_zero", ("shaded",), ()), ("normals_opposed", ("flip",), ()),
    # texture_shapes
] + [(n, ("shaded",), ()) for n, _ in A._shape_textures()] + [(n, ("shaded",), ()) for n in ("uv_plus_0", "uv_minus_0", "uv_on_texel_edge", "uv_on_texel_edge_outside", "uv_4096", "handle_past_the_table")]
_count.B = None


@pytest.mark.parametrize("frame", A.FRAMES, ids=[f"{w}x{h}" for w, h in A.FRAMES])
def test_every_class_shows_its_branches(records, oracle_mod, frame):
    _count.B = oracle_mod.BRANCH
    rec, _ = records
    short = []
    for name, need, avoid in CLAIMS:
        n = _count(rec, frame, (name,), need)
        if n < FLOOR:
            short.append(f"{name}: {'+'.join(need)} in {n} hits")
        for a in avoid:
            k = _count(rec, frame, (name,), (a,))
            if k:
                short.append(f"{name}: {a} in {k} hits, expected never")
    # tint from outside AND from inside; opposed normals flip without fromInside
    for name in ("tint_0", "tint_1"):
        if _count(rec, frame, (name,), ("bsdf2",), ("inside",)) < FLOOR:
            short.append(f"{name}: transmissive from outside")
    if _count(rec, frame, ("normals_opposed",), ("flip",), ("inside",)) < FLOOR:
        short.append("normals_opposed: flip without fromInside")
    assert not short, "; ".join(short)


@pytest.mark.parametrize("frame", A.FRAMES, ids=[f"{w}x{h}" for w, h in A.FRAMES])
def test_case_specific_witnesses(records, oracle_mod, frame):
    _count.B = B = oracle_mod.BRANCH
    rec, _ = records

    def only(cid):
        return {k: v for k, v in rec.items() if k == (cid, frame)}
    # the stack: six skipped layers, then the opaque base in the seventh and last bounce of the default depth
    sc, fl, what, _, _ = rec[("one_A", frame)]
    mesh = (what[0] & 0xFFFF).astype(np.int64) - 1
    layers = [k for k, n in enumerate(sc.swatch_name) if n.startswith("stack_layer_")]; base = sc.swatch_name.index("stack_base")
    six = np.all([((fl[0, b] & B["alpha_skip"]) != 0) & np.isin(mesh[b], layers) for b in range(6)], 0) & (mesh[6] == base) & ((fl[0, 6] & B["alpha_skip"]) == 0)
    n_stack = sum(int((np.all([((r[1][0, b] & B["alpha_skip"]) != 0) for b in range(6)], 0) & (((r[2][0, 6] & 0xFFFF).astype(np.int64) - 1) == r[0].swatch_name.index("stack_base"))).sum())
                  for (cid, fr), r in rec.items() if fr == frame and r[1].shape[1] >= 7 and "stack_base" in r[0].swatch_name)
    assert n_stack >= FLOOR and six.sum() >= 1, (n_stack, int(six.sum()))
    # frame_edges under the parallel camera: N.z = +1/1023 does not flip, N.z = -1/1023 flips (bounce 0: every primary ray is (0, 0, -1))
    assert _count(only("parallel_pos"), frame, ("perpendicular_pos",), ("shaded",), ("flip",), bounce=0) >= FLOOR and _count(only("parallel_pos"), frame, ("perpendicular_pos",), ("flip",), bounce=0) == 0
    assert _count(only("parallel_neg"), frame, ("perpendicular_neg",), ("flip",), bounce=0) >= FLOOR
    # cosTheta == 0 exactly: vertex normals (1, 0, 1) decode to |x| == |z|, the ray is (s, 0, -s): every primary hit has cosTheta == 0 and is NOT flipped (`cosTheta < 0`)
    n_px = frame[0] * frame[1]
    assert _count(only("parallel_exact"), frame, ("perpendicular_exact",), ("cos_zero",), ("flip", "inside"), bounce=0) == n_px
    # instance_frames: the scaled (transform 16) and the mirrored (17) instance are shaded, from outside and from inside
    for cid in ("inst_x_loop_A", "inst_x_tlas_A"):
        for x in (16, 17):
            assert _count(only(cid), frame, None, ("shaded",), xform=x) >= FLOOR, (cid, x)
        assert _count(only(cid), frame, None, ("inside",), xform=16) + _count(only(cid), frame, None, ("inside",), xform=17) >= FLOOR, cid
        assert _count(only(cid), frame, None, ("bsdf2",), xform=17) >= FLOOR, cid
    # light_edges
    def lights(cid, need, avoid=()):
        sc, fl, what, _, _ = rec[(cid, frame)]
        sel = (what >> 31) == 1
        for n in need:
            sel &= (fl & B[n]) != 0
        for n in avoid:
            sel &= (fl & B[n]) == 0
        return sel
    assert lights("lights_first", ("light",))[0, 0].sum() >= FLOOR                                     # the light is hit first
    assert (lights("lights_first", ("light",))[0, 0] & (rec[("lights_first", frame)][2][0, 0] == 0x80000000)).sum() >= FLOOR
    assert lights("lights_inside", ("light", "inside"))[0, 0].sum() >= FLOOR                           # camera inside the sphere
    assert (lights("lights_small", ("light",))[0, 0] & (rec[("lights_small", frame)][2][0, 0] == 0x80000001)).sum() >= FLOOR      # radius 2^-10
    assert lights("lights_A", ("light",)).sum() >= FLOOR
    assert (rec[("lights_off", frame)][1] & B["light"]).sum() == 0 and (rec[("one_A", frame)][1] & B["light"]).sum() == 0       # lights present, DoTraceLights 0
    # dark_throughput
    sc, fl, what, img, _ = rec[("dark_no_roulette", frame)]
    assert ((fl & B["throughput_subnormal"]) != 0).sum() >= FLOOR and ((fl & B["throughput_zero"]) != 0).sum() >= FLOOR
    rgb = img[..., :3]
    assert ((np.abs(rgb) < FLT_MIN) & (rgb != 0)).any(), "no subnormal radiance"
    assert (fl & B["sky"]).sum() == 0 and (rec[("closed_A", frame)][1] & B["sky"]).sum() == 0          # closed: nothing reaches the sky
    assert ((rec[("dark_roulette", frame)][1] & B["roulette"]) != 0).sum() >= FLOOR
    assert ((rec[("one_A", frame)][1] & B["sky"]) != 0).sum() >= FLOOR and ((rec[("one_A", frame)][1] & B["roulette"]) != 0).sum() >= FLOOR


def test_every_class_but_non_finite_is_finite(records):
    _, finite = records
    bad = [k for k, v in finite.items() if not v]
    assert not bad, bad[:5]


def test_non_finite_holds_an_infinity_and_a_nan(native_builder, oracle_mod):
    sc = A.cached_room("non_finite", native_builder)
    for (w, h) in A.FRAMES:
        o, _ = A.render_oracle(oracle_mod, sc, A.camera("A", w, h), w, h, {}, frames=2)
        img = o.image(0); o.close()
        assert np.isinf(img).any() and np.isnan(img).any(), (w, h)


def test_sky_ties_are_ties(native_builder, oracle_mod):
    """every ray of a sky_ties frame goes straight into the sky; the direction along (1, 1, 0) has two bit-equal components, along (1, 1, 1) three equal magnitudes"""
    B = oracle_mod.BRANCH
    for cid, size, d in A.sky_cases():
        sc = A.cached_room("sky_probe", native_builder, size)
        assert sc.sky_faces.shape[1] == size and len(np.unique(sc.sky_faces[..., :3])) == 18 * size * size
        pf = A.parallel_camera((0.0, 0.0, 0.0), d)
        v = AR.primary_direction(pf)
        nz = v[np.float32(d) != 0]
        assert (np.abs(nz).view(np.uint32) == np.abs(nz).view(np.uint32)[0]).all() and (v[np.float32(d) == 0] == 0).all(), (cid, v)
        o, (fl, what) = A.render_oracle(oracle_mod, sc, pf, 8, 8, {}, record=True)
        assert ((fl[0, 0] & B["sky"]) != 0).all() and np.isfinite(o.image(0)).all(), cid
        o.close()


def test_inputs_are_on_their_boundaries(native_builder):
    sc = A.cached_room("one", native_builder)
    m = lambda n: sc.materials[sc.meshes["MaterialId"][sc.swatch_name.index(n)]]      # noqa: E731
    assert m("alpha_equals_cutoff")["AlphaCutoff"] == np.float32(0.5) and (m("alpha_equals_cutoff")["BaseColorFactor"] >> 24) == 255
    t = sc.textures[int(m("alpha_equals_cutoff")["BaseColorTexture"]) - 1]; assert t.data.shape == (1, 1, 4) and t.data[0, 0, 3] == np.float32(0.5)
    t = sc.textures[int(m("alpha_ulp_below_cutoff")["BaseColorTexture"]) - 1]; assert t.data[0, 0, 3] == np.nextafter(np.float32(0.5), np.float32(0))
    assert m("cutoff_above_2")["AlphaCutoff"] == np.nextafter(np.float32(2), np.float32(3))
    assert int(m("handle_past_the_table")["BaseColorTexture"]) == len(sc.textures) + 1
    # texture coordinates: constant over the swatch (all three corners equal: the interpolation is exact up to b0 + b1 + b2 rounding of equal values), on texel edges
    for name, uv in (("uv_plus_0", (0.0, 0.0)), ("uv_minus_0", (-0.0, -0.0)), ("uv_on_texel_edge", (0.5, 0.5)), ("uv_on_texel_edge_outside", (-1.5, 2.5)), ("uv_4096", (4096.0, 4096.0))):
        k = sc.swatch_name.index(name); tr = sc.blas_triangles[sc.blas_triangles["MeshId"] == k]
        tc = sc.vertices["TexCoord"][np.stack([tr["X"], tr["Y"], tr["Z"]], 1).reshape(-1)]
        assert (tc.view(np.uint32) == np.float32(uv).view(np.uint32)).all(), name
    for u, wdt in ((0.5, 5), (0.5, 1), (-1.5, 5), (2.5, 1), (2.5, 5), (-1.5, 1)):
        x = np.float32(u) * np.float32(wdt) - np.float32(0.5); assert x == np.floor(x)
    # every swatch is a closed box of 12 triangles with its own mesh and material; coordinates dyadic (multiples of 1/64)
    assert len(np.unique(sc.meshes["MaterialId"])) == len(sc.meshes) == len(sc.swatch_name)
    assert (np.bincount(sc.blas_triangles["MeshId"]) >= 12).all()
    assert (sc.vertex_positions * 64 == np.round(sc.vertex_positions * 64)).all()
    x = A.cached_room("inst_x", native_builder)
    assert len(x.blas_instances) == 18 and np.linalg.det(x.mesh_transforms[17]["Model"][:, :3].astype(np.float64)) < 0
    sv = np.linalg.svd(x.mesh_transforms[16]["Model"][:, :3].astype(np.float64), compute_uv=False); assert np.allclose(sv, (4.0, 1.0, 0.25))
    assert A.REGRESSION_SURFACES == {} or all(len(v) == 4 for v in A.REGRESSION_SURFACES.values())


def test_the_branch_record_changes_nothing(native_builder, oracle_mod):
    """hook off / on: image, AOVs, ray records, queue and statistics are the same bytes"""
    sc = A.cached_room("one", native_builder); w, h = 67, 35
    out = []
    for record in (False, True):
        o, _ = A.render_oracle(oracle_mod, sc, A.camera("A", w, h), w, h, {"OutputAOVs": 1, "SamplesPerPixel": 2, "DoTraceLights": 1}, frames=2, record=record)
        out.append((o.image(0).tobytes(), o.image(1).tobytes(), o.image(2).tobytes(), o.rays().tobytes(), o.alive_queue().tobytes(), o.stats()["rays_traced"]))
        o.close()
    assert out[0] == out[1]


def test_planted_frames_hold_a_draw_equal_to_the_chance(native_builder, oracle_mod):
    """every planted sample index shows a tie in the branch record, and together they show both kinds: the BSDF choice and the roulette"""
    B = oracle_mod.BRANCH
    sc = A.cached_room("one", native_builder); w, h = 64, 64
    kinds = set()
    for s in A.TIE_SAMPLES:
        o, (fl, _) = A.render_oracle(oracle_mod, sc, A.camera("A", w, h), w, h, {}, record=True, sequence=s)
        o.close()
        here = {k for k in ("chance_tie", "roulette_tie") if ((fl & B[k]) != 0).any()}
        assert here, s
        kinds |= here
    assert kinds == {"chance_tie", "roulette_tie"}
    found = A.find_ties(oracle_mod, native_builder, A.TIE_SAMPLES[0], A.TIE_SAMPLES[0] + 1)
    assert found and found[0][0] == A.TIE_SAMPLES[0] and found[0][1] == "chance_tie"


def test_shadow_occluders_and_planted_pixels_are_exercised(native_builder, oracle_mod):
    """CPU witnesses of the shadow cases: every planted kind covers at least 8 pixels, and switching one occluder off (or, for the box at alpha == cutoff, ON) changes the
    oracle's visibility in at least FLOOR pixels — so shadow rays do cross each of them: every textured box (wrap modes), the five blend layers, the box at alpha == cutoff
    (transparent as built), and the second light between fragments and the target."""
    from idkengine_amd import gputypes as T
    sc = A.shadow_room(native_builder)
    for (w, h) in A.FRAMES:
        plain = A.cached_room("inst_x", native_builder)
        cam, depth, normal, planted = A.shadow_gbuffer(sc, w, h, lambda r: oracle_mod.trace_rays(plain, r), raster=plain)
        assert all(n >= 8 for _, n in planted.values()), planted
        p = T.ShadowParams.make(cam.inv_proj_view, w, h, light_index=A.SHADOW_TARGET, samples=4, noise_index=0)
        base = oracle_mod.trace_shadows(sc, p, depth, normal)
        assert (base[planted["away"][0]][depth[planted["away"][0]] < 1.0] == 0.0).all()
        mats = sc.materials.copy(); lights = sc.lights.copy()
        try:
            groups = [[n] for n in sc.swatch_name if n.startswith("shadow_alpha_")] + [[n for n in sc.swatch_name if n.startswith("shadow_blend_layer_")]]
            for names in groups:
                sc.materials = mats.copy()
                for n in names:
                    m = sc.meshes["MaterialId"][sc.swatch_name.index(n)]
                    if n == "shadow_alpha_equals_cutoff":
                        sc.materials["AlphaCutoff"][m] = np.nextafter(np.float32(0.5), np.float32(0))       # one ulp lower: now an occluder
                    else:
                        sc.materials["AlphaCutoff"][m] = A.ABOVE_TWO                                         # never an occluder
                v = oracle_mod.trace_shadows(sc, p, depth, normal)
                assert (v != base).sum() >= FLOOR, (names, w, h, int((v != base).sum()))
            sc.materials = mats.copy()
            sc.lights = lights.copy(); sc.lights["Position"][A.SHADOW_BLOCKER] = (50.0, 50.0, 50.0)
            v = oracle_mod.trace_shadows(sc, p, depth, normal)
            assert (v != base).sum() >= FLOOR, ("blocker light", w, h)
        finally:
            sc.materials = mats; sc.lights = lights
