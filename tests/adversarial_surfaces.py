"""Adversarial SURFACES for the code that runs after a hit (numpy + idkengine_amd.scenes only, deterministic): ShadeHit behind k_shade_first / k_shade / k_shade_last +
k_restore_last / k_trace_fused, k_final_draw and the surface loop of k_shadows.  Every parameter sits ON a boundary of the shading instead of inside an interval.
tests/test_adversarial_surfaces_ref.py proves on the CPU, with the oracle's branch record, that each class takes the branches it was built for;
tests/test_gpu_adversarial_surfaces.py holds every kernel variant to the oracle on them, byte for byte.

The swatch room: two facing walls in the planes z = -2 and z = +2, each an 8 x 8 grid of swatches on dyadic coordinates (cell 1/2, swatch 7/16, thickness 1/8).  Every swatch is
a closed box of 12 triangles with its own GpuMesh and GpuMaterial — rays enter AND leave it — and carries a class and a name (swatch_table).  Cameras stand at the origin between
the walls: "A" looks at z = -2, "B" at z = +2, "parallel" sends every primary ray along (0, 0, -1).  Forms (room(form, builder)):
  one      one BLAS
  inst     one BLAS per swatch row (16), identity transforms; rendered with UseTlas 0 and 1
  inst_x   inst + two more instances of a swatch row: under the non-uniform scale (4, 1, 1/4) turned 23 degrees about Y, and under a mirror (negative determinant)
  closed   one + backing plates and four more walls: nothing reaches the sky (classes dark_throughput)
  dark     closed with every albedo 1/255 and one emissive swatch: throughput (1/255)^k walks through the subnormal range ((1/255)^16 ~ 3e-39) to exact 0.  The diffuse
           direction of a bounce is a function of the queue slot, and here no ray ever dies, so paths are regular and few reach the swatch late; its emission is therefore
           (1, 2^-110, 2^-126): emission x throughput is subnormal in blue from the first bounce on, in green from the fourth
  non_finite  one, with an emissive swatch whose emission overflows to +inf (factor 1e30 x texel 1e30) and black swatches (throughput exactly 0): inf, and inf * 0 = NaN
The sky is 2 x 2 texels per face, all 24 distinct; two sphere lights, one of them touching a swatch of wall A.

Kept out, and why:
  * zero tangents, vertex normals that cancel in the interpolation, a light of radius 0: the reference's own shader is NaN by construction there (normalize(0), x / 0) — nothing
    to hold the product to;
  * texture coordinates with |u * width| >= 2^31: the float -> int conversion of the texel index is undefined in the oracle's C++ (and in GLSL), so the oracle has no answer;
  * RayTracingSamples = 0 for the shadow kernel: include/idkpt.h admits only >= 1;
cosTheta == 0 exactly: SR11G11B10 has no code for 0 but holds +-1 exactly, so vertex normals (1, 0, 1) decode to |x| == |z| bit for bit and normalize keeps them equal; the
free-standing swatch "perpendicular_exact" carries them, and a parallel camera along (1, 0, -1) from the origin (case parallel_exact) gives (-s a + 0 b) + s a == 0: not flipped.
"perpendicular_pos" / "perpendicular_neg" (N.z = +-1/1023 under the (0, 0, -1) camera) are the two sides next to it: one flips, the other does not.
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from idkengine_amd import scenes as S  # noqa: E402
from idkengine_amd import gputypes as T  # noqa: E402
import adversarial_rays as AR  # noqa: E402

f32 = np.float32
CELL, MARGIN, THICK, WALL = 0.5, 1.0 / 32.0, 0.125, 2.0
CLASSES = ("alpha_edges", "chance_edges", "clamp_edges", "roughness_edges", "volume_edges", "frame_edges", "instance_frames", "texture_shapes", "light_edges", "dark_throughput",
           "sky_ties", "non_finite", "filler", "shell")
FRAMES = ((64, 64), (67, 35))
BELOW_HALF = float(np.nextafter(f32(0.5), f32(0.0)))
ABOVE_TWO = float(np.nextafter(f32(2.0), f32(3.0)))

# Swatches or pixels that once exposed a difference between kernel and oracle, by name: {"name": (form, camera, (width, height), (x, y) or swatch name)}.
REGRESSION_SURFACES = {
}


# ----------------------------------------------------------------------------------------------------------------- textures
def _tex(data, ws=0, wt=0, filt=0):
    return T.TextureImage(np.asarray(data, np.float32), ws, wt, filt)


def _const(rgba):
    return _tex(np.float32(rgba).reshape(1, 1, 4))


def _shape_textures():
    """1 x 1, 1 x 5 and 5 x 1 float images under every wrap mode x filter: 18 images, texels distinct, in [0.2, 1]"""
    rng = np.random.default_rng(19)
    out = []
    for (h, w) in ((1, 1), (1, 5), (5, 1)):
        for wrap in (T.IDKPT_WRAP_REPEAT, T.IDKPT_WRAP_CLAMP_TO_EDGE, T.IDKPT_WRAP_MIRRORED_REPEAT):
            for filt in (T.IDKPT_FILTER_LINEAR, T.IDKPT_FILTER_NEAREST):
                d = rng.uniform(0.2, 1.0, (h, w, 4)).astype(np.float32); d[..., 3] = 1.0
                out.append((f"{w}x{h}_wrap{wrap}_filter{filt}", _tex(d, wrap, wrap, filt)))
    return out


# ----------------------------------------------------------------------------------------------------------------- swatch specifications
def _spec(cls, name, mat=None, mesh=None, tex=None, uv="planar", normals="face", stack=0):
    return {"cls": cls, "name": name, "mat": mat or {}, "mesh": mesh or {}, "tex": tex or {}, "uv": uv, "normals": normals, "stack": stack}


def _glass(**kw):
    d = dict(base_color=(0.9, 0.8, 0.7, 1.0), transmission=1.0, roughness=0.0, ior=1.5, volumetric=True)
    d.update(kw)
    return d


def wall_a_specs():
    """the 55 boundary swatches of wall A (class, name, material, mesh, textures by slot) + fillers to 64"""
    s = []
    half = _const((1.0, 1.0, 1.0, 0.5)); below = _const((1.0, 1.0, 1.0, BELOW_HALF)); zero_a = _const((1.0, 1.0, 1.0, 0.0))
    col = (0.7, 0.6, 0.5, 1.0)
    # --- alpha_edges: `sAlpha < alphaCutoff`, `sAlphaCutoff == 2.0f`
    s += [_spec("alpha_edges", "cutoff_0", dict(base_color=col, alpha_cutoff=0.0)),
          _spec("alpha_edges", "alpha_equals_cutoff", dict(base_color=(0.7, 0.6, 0.5, 1.0), alpha_cutoff=0.5), tex={"BaseColorTexture": half}),          # 0.5 * (255 / 255) == 0.5: kept
          _spec("alpha_edges", "alpha_ulp_below_cutoff", dict(base_color=col, alpha_cutoff=0.5), tex={"BaseColorTexture": below}),                      # skipped
          _spec("alpha_edges", "cutoff_1_alpha_1", dict(base_color=col, alpha_cutoff=1.0)),
          _spec("alpha_edges", "blend_alpha_0", dict(base_color=col, alpha_cutoff=2.0), tex={"BaseColorTexture": zero_a}),
          _spec("alpha_edges", "blend_alpha_1", dict(base_color=col, alpha_cutoff=2.0)),
          _spec("alpha_edges", "cutoff_above_2", dict(base_color=col, alpha_cutoff=ABOVE_TWO)),                                                         # not blend: everything skipped
          _spec("alpha_edges", "stack_base", dict(base_color=(0.9, 0.3, 0.2, 1.0)), stack=3)]                                                           # three skipped boxes = six skipped layers in front
    # --- chance_edges: `metallic > rnd`, `metallic + transmission > rnd`, f0
    s += [_spec("chance_edges", "metallic_1", dict(base_color=col, metallic=1.0, roughness=0.3)),
          _spec("chance_edges", "transmission_1", _glass()),
          _spec("chance_edges", "both_1", _glass(metallic=1.0)),                                                                                         # diffuse chance -1
          _spec("chance_edges", "both_0", dict(base_color=col, metallic=0.0, transmission=0.0)),
          _spec("chance_edges", "ior_equals_previous", dict(base_color=col, ior=1.0, metallic=0.0, roughness=0.5)),                                      # f0 == 0 from outside
          _spec("chance_edges", "ior_1_both_sides", _glass(ior=1.0)),
          _spec("chance_edges", "ior_1e6", _glass(ior=1e6)),
          _spec("chance_edges", "ior_bias_below_1", _glass(ior=1.25), dict(IORBias=-0.5))]
    # --- clamp_edges: the five clamps of SurfaceApplyModificatons
    base = dict(base_color=col, metallic=0.25, roughness=0.25, transmission=0.25, ior=1.5, volumetric=True, absorbance=(0.5, 0.5, 0.5))
    for b in ("SpecularBias", "RoughnessBias", "TransmissionBias", "IORBias"):
        s += [_spec("clamp_edges", f"{b}_plus_10", dict(base), {b: 10.0}), _spec("clamp_edges", f"{b}_minus_10", dict(base), {b: -10.0})]
    s += [_spec("clamp_edges", "AbsorbanceBias_plus_10", _glass(absorbance=(0.5, 0.5, 0.5)), dict(AbsorbanceBias=(10.0, 10.0, 10.0))),
          _spec("clamp_edges", "AbsorbanceBias_minus_10", _glass(absorbance=(0.5, 0.5, 0.5)), dict(AbsorbanceBias=(-10.0, -10.0, -10.0)))]
    s += [_spec("clamp_edges", "lands_on_1", dict(base), dict(SpecularBias=0.75, RoughnessBias=0.75, TransmissionBias=0.75)),
          _spec("clamp_edges", "lands_on_0", dict(base), dict(SpecularBias=-0.25, RoughnessBias=-0.25, TransmissionBias=-0.25)),
          _spec("clamp_edges", "negative_zero_biases", dict(base_color=col, metallic=0.0, roughness=0.0, transmission=0.0),
                dict(SpecularBias=-0.0, RoughnessBias=-0.0, TransmissionBias=-0.0, IORBias=-0.0, EmissiveBias=-0.0, AbsorbanceBias=(-0.0, -0.0, -0.0))),
          _spec("clamp_edges", "absorbance_below_0", _glass(absorbance=(0.5, 0.5, 0.5)), dict(AbsorbanceBias=(-1.0, 0.0, 1.0))),
          _spec("clamp_edges", "emissive_bias", dict(base_color=col), dict(EmissiveBias=0.5))]
    # --- roughness_edges: gmix with factor 0 and 1 under each BSDF type
    for r in (0.0, 1.0):
        s += [_spec("roughness_edges", f"diffuse_r{int(r)}", dict(base_color=col, roughness=r)),
              _spec("roughness_edges", f"specular_r{int(r)}", dict(base_color=col, metallic=1.0, roughness=r)),
              _spec("roughness_edges", f"transmissive_r{int(r)}", _glass(roughness=r))]
    # --- volume_edges: absorption, gexp's -87 branch, refract's k < 0, thin walls, the tint
    s += [_spec("volume_edges", "absorbance_0", _glass(absorbance=(0.0, 0.0, 0.0))),
          _spec("volume_edges", "absorbance_straddles_87", _glass(absorbance=(600.0, 660.0, 720.0))),                                                    # T in [1/8, 0.2] inside: -a T from -75 to -144
          _spec("volume_edges", "absorbance_1e30", _glass(absorbance=(1e30, 1e30, 1e30))),
          _spec("volume_edges", "tir_ior_1_5", _glass(ior=1.5, roughness=0.0)),
          _spec("volume_edges", "tir_ior_2_4", _glass(ior=2.4, roughness=0.6)),
          _spec("volume_edges", "thin_walled", _glass(volumetric=False)),
          _spec("volume_edges", "tint_0", _glass(), dict(TintOnTransmissive=0)),
          _spec("volume_edges", "tint_1", _glass(), dict(TintOnTransmissive=1)),
          _spec("volume_edges", "thin_walled_tint_0", _glass(volumetric=False), dict(TintOnTransmissive=0))]
    # --- frame_edges: the TBN, the normal map, the flip
    rng = np.random.default_rng(23)
    nm = rng.uniform(0.2, 0.8, (2, 2, 4)).astype(np.float32)
    for k, st in enumerate((0.0, 1.0, 2.0, -1.0)):
        s.append(_spec("frame_edges", f"normal_map_strength_{st:g}", dict(base_color=col, metallic=0.5, roughness=0.3), dict(normal_map_strength=st), {"NormalTexture": _tex(nm)}))
    for name, rg in (("texel_half", (0.5, 0.5)), ("texel_one", (1.0, 1.0)), ("texel_zero", (0.0, 0.0))):                                               # (1, 1): radicand -1, max -> 0
        s.append(_spec("frame_edges", f"normal_{name}", dict(base_color=col, metallic=0.5, roughness=0.3), dict(normal_map_strength=1.0), {"NormalTexture": _const((rg[0], rg[1], 0.0, 1.0))}))
    s += [_spec("frame_edges", "normals_opposed", dict(base_color=col, metallic=0.5, roughness=0.3), normals="opposed"),                                 # flip without fromInside
          _spec("frame_edges", "perpendicular_pos", dict(base_color=col, metallic=0.5, roughness=0.3), normals="perp_pos"),
          _spec("frame_edges", "perpendicular_neg", dict(base_color=col, metallic=0.5, roughness=0.3), normals="perp_neg")]
    k = 0
    while len(s) < 64:
        s.append(_spec("filler", f"filler_a{k}", dict(base_color=(0.3 + 0.05 * (k % 8), 0.8 - 0.04 * k, 0.5, 1.0), roughness=0.5 + 0.04 * k))); k += 1
    assert len(s) == 64
    s[7], s[27] = s[27], s[7]                 # the stack stands in the middle of the wall: camera A's rays cross all six layers
    return s


def wall_b_specs():
    """texture_shapes on wall B; the rest of the wall repeats wall A's boundary swatches in another order (camera B sees them at other angles)"""
    s = []
    for name, t in _shape_textures():
        s.append(_spec("texture_shapes", name, dict(base_color=(1.0, 1.0, 1.0, 1.0), emissive=(0.5, 0.5, 0.5)), tex={"BaseColorTexture": t, "EmissiveTexture": t, "MetallicRoughnessTexture": t}))
    five = _shape_textures()[6][1]                                                                                                                      # 5 x 1, repeat, linear
    five_t = _shape_textures()[12][1]                                                                                                                   # 1 x 5, repeat, linear
    s += [_spec("texture_shapes", "uv_plus_0", dict(base_color=(1.0, 1.0, 1.0, 1.0)), tex={"BaseColorTexture": five}, uv=(0.0, 0.0)),
          _spec("texture_shapes", "uv_minus_0", dict(base_color=(1.0, 1.0, 1.0, 1.0)), tex={"BaseColorTexture": five_t}, uv=(-0.0, -0.0)),
          _spec("texture_shapes", "uv_on_texel_edge", dict(base_color=(1.0, 1.0, 1.0, 1.0)), tex={"BaseColorTexture": five, "EmissiveTexture": five_t}, uv=(0.5, 0.5)),      # 0.5 * 5 - 0.5 == 2, 0.5 * 1 - 0.5 == 0
          _spec("texture_shapes", "uv_on_texel_edge_outside", dict(base_color=(1.0, 1.0, 1.0, 1.0)), tex={"BaseColorTexture": five, "EmissiveTexture": five_t}, uv=(-1.5, 2.5)),
          _spec("texture_shapes", "uv_4096", dict(base_color=(1.0, 1.0, 1.0, 1.0)), tex={"BaseColorTexture": five, "EmissiveTexture": five_t}, uv=(4096.0, 4096.0)),
          _spec("texture_shapes", "handle_past_the_table", dict(base_color=(0.6, 0.7, 0.8, 1.0)), tex={"BaseColorTexture": "PAST"})]
    a = [x for x in wall_a_specs() if x["cls"] != "filler"]
    k = 0
    while len(s) < 64:
        src = a[(7 * k + 3) % len(a)]; k += 1
        if src["stack"]:
            continue
        s.append(dict(src, name=src["name"] + "_b"))
    return s


# ----------------------------------------------------------------------------------------------------------------- geometry
def _box(lo, hi):
    return S._box_faces(lo, hi, with_bottom=True)


def _swatch_mesh(spec, lo, hi, textures):
    """MeshInput of one swatch box [lo, hi]"""
    p, idx, nrm, tan = S.flat_shaded(_box(lo, hi))
    if spec["normals"] == "opposed":
        nrm = -nrm
    elif spec["normals"] in ("perp_pos", "perp_neg"):
        nrm = np.tile(f32([1.0, 0.0, 0.001 if spec["normals"] == "perp_pos" else -0.001]), (len(nrm), 1)); tan = np.tile(f32([0.0, 1.0, 0.0]), (len(nrm), 1))
    elif spec["normals"] == "perp_exact":     # decodes to (1, 1/2047, 1): |x| == |z| bit for bit, and normalize keeps them equal
        nrm = np.tile(f32([1.0, 0.0, 1.0]), (len(nrm), 1)); tan = np.tile(f32([0.0, 1.0, 0.0]), (len(nrm), 1))
    if spec["uv"] == "planar":
        uv = np.stack([(p[:, 0] - lo[0]) / (hi[0] - lo[0]), (p[:, 1] - lo[1]) / (hi[1] - lo[1])], 1).astype(np.float32)
    else:
        uv = np.tile(f32(spec["uv"]), (len(p), 1))
    m = S.make_material(**spec["mat"])
    for slot, t in spec["tex"].items():
        if isinstance(t, str):
            m[slot] = 0xFFFF                                                # "PAST": patched to len(table) + 1 once the table is complete
        else:
            textures.append(t); m[slot] = len(textures)
    return S.MeshInput(p, idx, m, nrm, tan, uv, dict(spec["mesh"]))


def _cells(specs, z_front, wall_sign):
    """(spec, lo, hi) per cell, row-major from the bottom left; rows are the BLASes of the instanced forms"""
    out = []
    for k, sp in enumerate(specs):
        i, j = k % 8, k // 8
        x0, y0 = -WALL + i * CELL + MARGIN, -WALL + j * CELL + MARGIN
        z = (z_front - THICK, z_front) if wall_sign > 0 else (z_front, z_front + THICK)
        out.append((sp, (x0, y0, z[0]), (x0 + CELL - 2 * MARGIN, y0 + CELL - 2 * MARGIN, z[1])))
    return out


SCALED_ROW, MIRRORED_ROW = 1, 5          # rows of wall A whose BLAS is instanced again in form inst_x


def extra_instance_matrices():
    """OpenTK-convention 4x4 of the two extra instances: scale (4, 1, 1/4), a 23-degree turn about Y and a move in front of wall A's lower rows; a mirror in x (determinant -1),
    moved in front of the upper rows"""
    sc = np.diag([4.0, 1.0, 0.25, 1.0]) @ S.rotation_y(23.0) @ S.translation((0.0, 0.75, -1.0))
    mi = np.diag([-1.0, 1.0, 1.0, 1.0]) @ S.translation((0.0, -0.75, 0.5))
    return sc, mi


EXACT_LO, EXACT_HI = (2.03125, -0.21875, -2.375), (2.46875, 0.21875, -2.25)     # the free-standing swatch perpendicular_exact: the ray from the origin along (1, 0, -1) meets its front face


def room(form, builder, sky_size=2, extra_blas=None):
    """The scene of one form + its swatch table: sc.swatch_class / sc.swatch_name per mesh id.  extra_blas(textures) -> (meshes, [(class, name)]): one more BLAS under the
    identity (instanced forms), its textures appended to the table."""
    textures, rows, table = [], [], []
    dark = form == "dark"
    for wall_sign, specs, zf in ((1, wall_a_specs(), -WALL), (-1, wall_b_specs(), WALL)):
        cells = _cells(specs, zf, wall_sign)
        for j in range(8):
            meshes = []
            for k in range(8 * j, 8 * j + 8):
                sp, lo, hi = cells[k]
                if dark:
                    lit = wall_sign > 0 and k == 27
                    sp = _spec("dark_throughput", "emissive" if lit else f"dark_{'a' if wall_sign > 0 else 'b'}{k}", dict(base_color=(1 / 255.0, 1 / 255.0, 1 / 255.0, 1.0), emissive=(1.0, 2.0 ** -110, 2.0 ** -126) if lit else (0, 0, 0)))
                elif form == "non_finite":
                    if (wall_sign > 0 and k in (27, 36)) or (wall_sign < 0 and k % 2 == 0):
                        sp = _spec("non_finite", f"emissive_inf_{k}", dict(base_color=(0.5, 0.5, 0.5, 1.0), emissive=(1e30, 1e30, 1e30)), tex={"EmissiveTexture": _const((1e30, 1e30, 1e30, 1.0))})
                    elif wall_sign > 0 and k % 3 == 0:
                        sp = _spec("non_finite", f"black_{k}", dict(base_color=(0.0, 0.0, 0.0, 1.0)))
                meshes.append(_swatch_mesh(sp, lo, hi, textures)); table.append((sp["cls"], sp["name"]))
                for n in range(sp["stack"] if not dark else 0):             # skipped boxes in front of the swatch: two skipped layers each
                    dz = 0.1875 * (n + 1)
                    l2, h2 = (lo[0], lo[1], lo[2] + dz), (hi[0], hi[1], hi[2] + dz)
                    lay = _spec("alpha_edges", f"stack_layer_{n}", dict(base_color=(0.2, 0.9, 0.4, 1.0), alpha_cutoff=ABOVE_TWO))
                    meshes.append(_swatch_mesh(lay, l2, h2, textures)); table.append((lay["cls"], lay["name"]))
            if wall_sign > 0 and j == 7:                                   # vertex normals (1, 0, 1) on every face: cosTheta == 0 exactly for the ray (s, 0, -s)
                sp = _spec("dark_throughput", "dark_exact", dict(base_color=(1 / 255.0, 1 / 255.0, 1 / 255.0, 1.0))) if dark else \
                    _spec("frame_edges", "perpendicular_exact", dict(base_color=(0.7, 0.6, 0.5, 1.0), metallic=0.5, roughness=0.3), normals="perp_exact")
                meshes.append(_swatch_mesh(sp, EXACT_LO, EXACT_HI, textures)); table.append((sp["cls"], sp["name"]))
            rows.append(meshes)
    if form in ("closed", "dark"):
        shell_col = (1 / 255.0,) * 3 + (1.0,) if dark else (0.6, 0.6, 0.6, 1.0)
        W = WALL + 0.5
        boxes = [((-W, -W, -W - 0.25), (W, W, -W)), ((-W, -W, W), (W, W, W + 0.25)), ((-W - 0.25, -W, -W), (-W, W, W)), ((W, -W, -W), (W + 0.25, W, W)),
                 ((-W, -W - 0.25, -W), (W, -W, W)), ((-W, W, -W), (W, W + 0.25, W))]                                                                     # two backing plates + four walls
        shell = []
        for lo, hi in boxes:
            shell.append(_swatch_mesh(_spec("shell", "shell", dict(base_color=shell_col)), lo, hi, textures)); table.append(("shell", "shell"))
        rows.append(shell)
    if extra_blas is not None:
        assert form in ("inst", "inst_x")
        extra, extra_table = extra_blas(textures)
        rows.append(extra); table += extra_table
    if form in ("inst", "inst_x"):
        sc = S.assemble([{"meshes": r} for r in rows], builder, build_tlas=False)
        if form == "inst_x":
            inst = np.zeros(len(rows) + 2, T.GpuBlasInstance)
            inst["BlasId"] = list(range(len(rows))) + [SCALED_ROW, MIRRORED_ROW]; inst["MeshTransformId"] = np.arange(len(rows) + 2)
            sc.blas_instances = inst
            sc.mesh_transforms = np.concatenate([sc.mesh_transforms] + [S.transform_from_matrix(m) for m in extra_instance_matrices()])
        S.rebuild_tlas(sc, builder)
    else:
        sc = S.assemble([{"meshes": [m for r in rows for m in r]}], builder)
    for slot in ("BaseColorTexture", "MetallicRoughnessTexture", "NormalTexture", "EmissiveTexture", "TransmissionTexture"):
        sc.materials[slot][sc.materials[slot] == 0xFFFF] = len(textures) + 1                                                                             # one past the table: white
    sc.textures = textures
    sc.sky_faces = sky(sky_size)
    sc.lights = S.make_lights([((-0.25, 0.25, -WALL + 0.25), 0.25, (6.0, 5.0, 4.0)),        # touches wall A (its lowest point in z is the wall's front plane)
                               ((0.5, -0.5, 1.0), 2.0 ** -10, (300.0, 200.0, 100.0))])     # radius 2^-10
    sc.swatch_class = [c for c, _ in table]; sc.swatch_name = [n for _, n in table]
    return sc


def sky(size):
    """6 x size x size texels, all distinct"""
    n = 6 * size * size
    v = (0.25 + np.arange(3 * n, dtype=np.float64) / (3 * n)).reshape(6, size, size, 3)
    out = np.ones((6, size, size, 4), np.float32); out[..., :3] = v
    return out


def sky_probe(builder, size):
    """One swatch row far below the camera: every ray of the sky_ties frames misses it"""
    tex = []
    cells = _cells(wall_a_specs()[56:64] , -WALL, 1)
    meshes = [_swatch_mesh(sp, (lo[0], lo[1] - 50.0, lo[2]), (hi[0], hi[1] - 50.0, hi[2]), tex) for sp, lo, hi in cells]
    sc = S.assemble([{"meshes": meshes}], builder)
    sc.textures = tex; sc.sky_faces = sky(size)
    sc.swatch_class = ["filler"] * len(meshes); sc.swatch_name = [f"probe{k}" for k in range(len(meshes))]
    return sc


# ----------------------------------------------------------------------------------------------------------------- cameras (raw per-frame records)
def _record(cam):
    p = np.zeros(1, T.GpuPerFrameData)
    p["InvProjection"][0] = cam.inv_projection; p["InvView"][0] = cam.inv_view; p["ViewPos"][0] = cam.position
    return p


def camera(name, w, h):
    """GpuPerFrameData of a named camera"""
    if name == "A":
        return _record(S.Camera(w, h, position=(0.0, 0.0, 0.0), view_dir=(0.0, 0.0, -1.0), fovy_deg=90.0))
    if name == "B":
        return _record(S.Camera(w, h, position=(0.03125, -0.0625, 0.0), view_dir=(0.0, 0.0, 1.0), fovy_deg=90.0))
    if name == "A_near":                      # close to wall A's middle rows: the ragged frame's pixels are wide
        return _record(S.Camera(w, h, position=(0.0, 0.0, -0.75), view_dir=(0.0, 0.0, -1.0), fovy_deg=90.0))
    if name == "in_light":                    # inside the sphere of light 0
        return _record(S.Camera(w, h, position=(-0.25, 0.25, -WALL + 0.375), view_dir=(0.3, 0.1, 1.0), fovy_deg=90.0))
    if name == "at_small_light":              # 2^-8 in front of light 1 (radius 2^-10)
        return _record(S.Camera(w, h, position=(0.5, -0.5, 1.0 + 2.0 ** -8), view_dir=(0.0, 0.0, -1.0), fovy_deg=90.0))
    if name == "at_light":                    # light 0 fills the middle of the frame: the light is hit first
        return _record(S.Camera(w, h, position=(-0.25, 0.25, -0.5), view_dir=(0.0, 0.0, -1.0), fovy_deg=60.0))
    raise ValueError(name)


def parallel_camera(view_pos, direction=(0.0, 0.0, -1.0)):
    """AR.perframe("parallel") whose one primary direction is normalize(direction) in binary32: the -Z column of InvView is -direction"""
    iv = np.eye(4, dtype=np.float32); iv[2, :3] = -f32(direction)
    return AR.perframe("parallel", iv, view_pos)


def swatch_centre(sc, name):
    """world-space centre of the named swatch's box (identity-transform forms)"""
    k = sc.swatch_name.index(name)
    t = sc.blas_triangles[sc.blas_triangles["MeshId"] == k]
    p = sc.vertex_positions[np.stack([t["X"], t["Y"], t["Z"]], 1).reshape(-1)]
    return 0.5 * (p.min(0) + p.max(0))


SKY_DIRECTIONS = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1), "xy": (1, 1, 0), "xyz": (1, 1, 1), "-xyz": (-1, 1, 1)}


# ----------------------------------------------------------------------------------------------------------------- the cases of the GPU test
def cases():
    """[(case id, class the case is for, form, UseTlas, camera name or ("parallel", swatch) , settings overrides)] — each rendered at FRAMES; the variants of the GPU test are applied on top"""
    c = [("one_A", "all", "one", 0, "A", {}), ("one_B", "all", "one", 0, "B", {}), ("one_A_near", "all", "one", 0, "A_near", {}),
         ("inst_loop_A", "all", "inst", 0, "A", {}), ("inst_tlas_B", "all", "inst", 1, "B", {}),
         ("inst_x_loop_A", "instance_frames", "inst_x", 0, "A", {}), ("inst_x_tlas_A", "instance_frames", "inst_x", 1, "A", {}),
         ("parallel_pos", "frame_edges", "one", 0, ("parallel", "perpendicular_pos"), {}), ("parallel_neg", "frame_edges", "one", 0, ("parallel", "perpendicular_neg"), {}),
         ("parallel_exact", "frame_edges", "one", 0, ("exact",), {}),
         ("lights_A", "light_edges", "one", 0, "A", {"DoTraceLights": 1}), ("lights_first", "light_edges", "one", 0, "at_light", {"DoTraceLights": 1}),
         ("lights_inside", "light_edges", "one", 0, "in_light", {"DoTraceLights": 1}), ("lights_small", "light_edges", "one", 0, "at_small_light", {"DoTraceLights": 1}), ("lights_off", "light_edges", "one", 0, "at_light", {"DoTraceLights": 0}),
         ("closed_A", "dark_throughput", "closed", 0, "A", {}),
         ("dark_no_roulette", "dark_throughput", "dark", 0, "A", {"DoRussianRoulette": 0, "RayDepth": 20}), ("dark_roulette", "dark_throughput", "dark", 0, "A", {"DoRussianRoulette": 1, "RayDepth": 20})]
    return c


def case_camera(sc, cam, w, h):
    if isinstance(cam, tuple) and cam[0] == "exact":          # from the origin along (1, 0, -1): -rayDir = (-s, 0, s) against N = (a, b, a): (-s a + 0 b) + s a == 0
        return parallel_camera((0.0, 0.0, 0.0), (1.0, 0.0, -1.0))
    if isinstance(cam, tuple):
        c = swatch_centre(sc, cam[1])
        return parallel_camera((float(c[0]) + 0.03125, float(c[1]) + 0.015625, 0.0))
    return camera(cam, w, h)


# one setting or developer option at a time from the default: (id, developer options, settings overrides, frames, max batch or 0)
VARIANTS = [("default", {}, {}, 1, 0), ("defer_last0", {"defer_last": 0}, {}, 1, 0), ("defer_last1", {"defer_last": 1}, {}, 1, 0), ("fused2", {"fused": 2, "fused_shade_min": 1}, {}, 1, 0),
            ("sorting", {}, {"DoRaySorting": 1}, 1, 0), ("aovs", {}, {"OutputAOVs": 1}, 1, 0), ("spp3_one_batch", {}, {"SamplesPerPixel": 3}, 1, 3), ("spp3_one_at_a_time", {}, {"SamplesPerPixel": 3}, 1, 1),
            ("bounce_pixel_major0", {"bounce_pixel_major": 0}, {}, 1, 0), ("bounce_pixel_major2", {"bounce_pixel_major": 2}, {}, 1, 0), ("three_frames", {}, {}, 3, 0),
            ("depth1", {}, {"RayDepth": 1}, 1, 0), ("depth2", {}, {"RayDepth": 2}, 1, 0), ("depth7", {}, {"RayDepth": 7}, 1, 0), ("depth20", {}, {"RayDepth": 20}, 1, 0)]


def settings_key(base, ov, frames):
    d = dict(base); d.update(ov)
    return tuple(sorted(d.items())) + (("frames", frames),)


# ----------------------------------------------------------------------------------------------------------------- comparison
def pixel_class(sc, tri):
    """class and name of the swatch of each primary hit (triangle ids; 0xFFFFFFFF: "sky or light")"""
    hit = tri != 0xFFFFFFFF
    mesh = sc.blas_triangles["MeshId"][np.where(hit, tri, 0)]
    return [f"{sc.swatch_class[m]}/{sc.swatch_name[m]}" if h else "sky or light" for m, h in zip(mesh, hit)]


def _fields(pt_like):
    """every compared output as (name, (pixels, k) uint32 view)"""
    out = [("image", np.ascontiguousarray(pt_like["image"]).view(np.uint32).reshape(-1, 4))]
    r = pt_like["rays"]
    for f in r.dtype.names:
        out.append((f"rays.{f}", np.ascontiguousarray(r[f]).view(np.uint32).reshape(len(r), -1)))
    out += [("albedo", np.ascontiguousarray(pt_like["albedo"]).view(np.uint32).reshape(-1, 4)), ("normal", np.ascontiguousarray(pt_like["normal"]).view(np.uint32).reshape(-1, 4))]
    return out


def snapshot(p):
    """the compared outputs of a PathTracer or an OraclePathTracer as arrays"""
    is_gpu = hasattr(p, "Result")
    img = (lambda k: p.download(k)) if is_gpu else (lambda k: p.image(k))
    t, tri, bary = p.primary_hits()
    return {"image": img(0), "albedo": img(1), "normal": img(2), "rays": p.rays(), "alive": p.alive_queue(), "prim_t": t, "prim_tri": tri, "prim_bary": bary, "rays_traced": p.stats()["rays_traced"]}


def same_value(a, b):
    """The relaxed equality of class non_finite, elementwise on float32 arrays: equal bits, or both NaN, or both the same signed infinity.  x86 and the device produce default NaNs
    of opposite sign (inf * 0 is 0xFFC00000 on SSE, 0x7FC00000 on the device), and a NaN's payload is not part of binary32 arithmetic; everything finite still compares on bits."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.signbit(a) == np.signbit(b)))


def first_difference(got, want, sc, width, relaxed=False):
    """None, or a report naming the first differing pixel, the swatch class of its primary hit and the first differing field (got / want: snapshot())"""
    msgs = []
    if got["rays_traced"] != want["rays_traced"]:
        msgs.append(f"rays traced {got['rays_traced']} != {want['rays_traced']}")
    if len(got["alive"]) != len(want["alive"]) or (got["alive"] != want["alive"]).any():
        msgs.append(f"alive queue differs ({len(got['alive'])} / {len(want['alive'])} entries)")
    cls = pixel_class(sc, want["prim_tri"])
    best = None
    pairs = [("primary.tri", got["prim_tri"].reshape(-1, 1), want["prim_tri"].reshape(-1, 1), False), ("primary.T", got["prim_t"].reshape(-1, 1), want["prim_t"].reshape(-1, 1), True),
             ("primary.bary", got["prim_bary"], want["prim_bary"], True)]
    kinds = {"image": "f", "albedo": "f", "normal": "f"}; kinds.update({f"rays.{f}": got["rays"].dtype[f].base.kind for f in got["rays"].dtype.names})
    pairs += [(n, g, w, kinds[n] == "f") for (n, g), (_, w) in zip(_fields(got), _fields(want))]
    for name, g, w, is_float in pairs:
        if relaxed and is_float:                               # (is_float: by dtype, see below — integer fields always compare on bits)
            bad = ~same_value(g.view(np.float32), w.view(np.float32))
        else:
            bad = g.view(np.uint32) != w.view(np.uint32)
        rows = np.nonzero(bad.reshape(len(bad), -1).any(1))[0]
        if len(rows) and (best is None or rows[0] < best[0]):
            best = (int(rows[0]), name, g[rows[0]], w[rows[0]], len(rows))
    if best is not None:
        i, name, g, w, n = best
        show = (lambda v: v.view(np.float32).tolist()) if name != "primary.tri" else (lambda v: v.tolist())
        msgs.append(f"pixel ({i % width}, {i // width}) primary hit on {cls[i]}: field {name} is {show(g)!r} (bits {[hex(int(x)) for x in g.view(np.uint32).ravel()]}), the oracle has {show(w)!r} "
                    f"(bits {[hex(int(x)) for x in w.view(np.uint32).ravel()]}); {n} pixels differ in that field")
    return "; ".join(msgs) if msgs else None


# ----------------------------------------------------------------------------------------------------------------- shared drivers of the two test files
_ROOMS = {}


def cached_room(form, builder, sky_size=2):
    key = (form, sky_size, type(builder).__name__)
    if key not in _ROOMS:
        _ROOMS[key] = room(form, builder, sky_size) if form != "sky_probe" else sky_probe(builder, sky_size)
    return _ROOMS[key]


def sky_cases():
    """[(id, sky size, direction)]: 8 x 8 frames of one ray each, straight into the sky"""
    return [(f"sky{size}_{name}", size, d) for size in (1, 2, 5) for name, d in SKY_DIRECTIONS.items()]


def apply(settings, overrides):
    for k, v in overrides.items():
        setattr(settings.Gpu if hasattr(settings.Gpu, k) else settings, k, v)
    return settings


def render_oracle(O, sc, per_frame, w, h, overrides, frames=1, record=False, sequence=None):
    """the oracle's frame; record: (flags, what) of OraclePathTracer.set_branch_record for the first frame's samples; sequence: first index of idkptSetSampleSequence (stride 1)"""
    o = O.OraclePathTracer(sc, w, h); o.set_perframe_data(per_frame)
    apply(o.settings, overrides)
    if sequence is not None:
        o.set_sample_sequence(sequence, 1)
    rec = o.set_branch_record(o.settings.SamplesPerPixel) if record else None
    for _ in range(frames):
        o.render()
    return o, rec


# ----------------------------------------------------------------------------------------------------------------- draws that equal the chance
# `specularChance > rnd`, `specularChance + transmissionChance > rnd` and the roulette's `rnd01 > p` part from their `>=` forms only where the draw EQUALS the chance: rnd01 is
# float(pcg) * 2^-32, so that is a 2^-24 event per hit for a chance in [0.5, 1) and no material moves it.  The frames are planted instead: form "one", camera A, 64 x 64, default
# settings, one sample at these indices of idkptSetSampleSequence — found by find_ties over the indices 1 .. 30 000 (CPU only, about a minute), and proved by the reference test.
# They depend on the room as it is built here: a change of the swatch layout asks for a new search (the reference test fails if a planted frame holds no tie any more).
TIE_SAMPLES = (686, 12174, 20990, 4966, 4994)          # 686, 12174, 20990: BSDF-choice ties (primary hits on glass swatches); 4966, 4994: roulette ties


def find_ties(O, builder, first, last):
    """[(sample index, "chance_tie" | "roulette_tie", bounce, pixel)] of the planted frame for the sample indices first .. last - 1, from the oracle's branch record"""
    sc = cached_room("one", builder); w, h = FRAMES[0]
    o = O.OraclePathTracer(sc, w, h); o.set_perframe_data(camera("A", w, h))
    out = []
    for s in range(first, last):
        o.set_sample_sequence(s, 1)
        fl, _ = o.set_branch_record(1); o.render()
        for name in ("chance_tie", "roulette_tie"):
            for b, px in np.argwhere((fl[0] & O.BRANCH[name]) != 0):
                out.append((s, name, int(b), int(px)))
    o.close()
    return out


# ----------------------------------------------------------------------------------------------------------------- shadows
SHADOW_TARGET, SHADOW_BLOCKER = 0, 1


def _shadow_occluders(textures):
    """the occluder BLAS of shadow_room: (meshes, [(class, name)])"""
    alpha = np.ones((1, 5, 4), np.float32); alpha[0, :, 3] = (0.0, 0.25, 0.5, 0.75, 1.0)
    meshes, table = [], []
    for k, wrap in enumerate((T.IDKPT_WRAP_REPEAT, T.IDKPT_WRAP_CLAMP_TO_EDGE, T.IDKPT_WRAP_MIRRORED_REPEAT)):
        sp = _spec("alpha_edges", f"shadow_alpha_texture_wrap{wrap}", dict(base_color=(0.5, 0.5, 0.5, 1.0), alpha_cutoff=0.5), tex={"BaseColorTexture": _tex(alpha, wrap, wrap, k % 2)})
        x0 = -1.0 + 0.75 * k
        m = _swatch_mesh(sp, (x0, -1.5, -1.5), (x0 + 0.75, -0.75, -1.375), textures)
        m.uvs = (m.uvs * 3.0 - 1.0).astype(np.float32)                                   # u, v from -1 to 2: the wrap mode decides
        meshes.append(m); table.append((sp["cls"], sp["name"]))
    sp = _spec("alpha_edges", "shadow_alpha_equals_cutoff", dict(base_color=(0.5, 0.5, 0.5, 1.0), alpha_cutoff=0.5), tex={"BaseColorTexture": _const((1.0, 1.0, 1.0, 0.5))})
    meshes.append(_swatch_mesh(sp, (-1.5, 0.75, -1.5), (-0.75, 1.5, -1.375), textures)); table.append((sp["cls"], sp["name"]))
    for n in range(5):
        z = -1.5 + 0.0625 * n
        q = S._quad((0.75, 0.75, z), (1.5, 0.75, z), (1.5, 1.5, z), (0.75, 1.5, z))
        p, idx, nrm, tan = S.flat_shaded(q)
        meshes.append(S.MeshInput(p, idx, S.make_material((0.4, 0.5, 0.6, 159.0 / 255.0), alpha_cutoff=2.0), nrm, tan)); table.append(("alpha_edges", f"shadow_blend_layer_{n}"))
    return meshes, table


def shadow_room(builder):
    """inst_x + a BLAS of occluders floating between wall A and the target light: boxes whose alpha comes from a 5 x 1 texture (one per wrap mode, cutoff 0.5), a box whose alpha
    equals its cutoff (not an occluder: `alpha > cutoff`), five blend layers of alpha 159/255 (visibility 0.3765^k: 0.0200 after four, 0.0076 < 0.01 after the fifth).
    Light 0 is the target, light 1 lies between part of wall A and the target."""
    sc = room("inst_x", builder, extra_blas=_shadow_occluders)
    sc.lights = S.make_lights([((0.25, 0.25, -0.75), 0.25, (9.0, 9.0, 9.0)), ((0.125, 0.125, -1.375), 0.125, (3.0, 3.0, 3.0))])
    return sc


def shadow_gbuffer(sc, w, h, trace, raster=None):
    """(camera, depth, normal, planted) — S.gbuffer_from_hits of camera A's primary hits (trace(rays) -> RayHit), then planted pixels; planted: {kind: (row, number of pixels)}.
    raster: the scene `trace` ran on, if not sc — the room WITHOUT the occluder BLAS, as a rasterizer that keeps alpha-tested and blended geometry out of its G-buffer sees it:
    the fragments then lie on the wall BEHIND the occluders and their shadow rays cross them (seen from the camera the occluders would hide exactly those fragments).
    Row 0: depth exactly 1 (the kernel leaves the output alone).  The other kinds go to the four rows in which most view rays cross the target light's sphere (they also hit
    wall A): "away": normals facing away from the light; "perpendicular": normals perpendicular to the direction of the light to rounding (cosTheta about +-1e-8, either side of
    the `<= 0` test: the fragment position is rebuilt from depth in binary32); "inside" / "on": fragments inside the sphere / at distance == radius (to rounding) from its
    centre, in the columns whose view ray passes within 0.9 radius of the centre."""
    cam = S.Camera(w, h, position=(0.0, 0.0, 0.0), view_dir=(0.0, 0.0, -1.0), fovy_deg=90.0)
    rays = S.primary_ray_queries(cam, w, h)
    hits = trace(rays)
    depth, normal = S.gbuffer_from_hits(raster if raster is not None else sc, cam, w, h, rays, hits)
    depth = depth.copy(); normal = normal.copy()
    L = sc.lights[SHADOW_TARGET]["Position"].astype(np.float64); R = float(sc.lights[SHADOW_TARGET]["Radius"])
    d = rays["Direction"].astype(np.float64).reshape(h, w, 3); t = hits["T"].astype(np.float64).reshape(h, w)
    vp = cam.view @ cam.proj

    def depth_of(P):
        c = np.c_[P, np.ones(len(P))] @ vp
        return (c[:, 2] / c[:, 3]).astype(np.float32)
    s_all = d @ L
    through_all = np.linalg.norm(d * s_all[..., None] - L, axis=2) < 0.9 * R
    hit = (hits["Hit"] != 0).reshape(h, w)
    rows = [int(r) for r in np.argsort(-(through_all & hit).sum(1), kind="stable")[:4]]
    planted = {"depth_one": (0, w)}
    depth[0, :] = 1.0
    for row, kind in zip(rows[2:], ("away", "perpendicular")):
        P = d[row] * t[row][:, None]; to = L - P; to /= np.linalg.norm(to, axis=1, keepdims=True)
        if kind == "away":
            n = -to
        else:
            n = np.cross(to, np.float64([0.3, 0.5, 0.8])); n /= np.linalg.norm(n, axis=1, keepdims=True)
        normal[row] = np.where(hit[row][:, None], S.oct_encode(n), normal[row])
        planted[kind] = (row, int(hit[row].sum()))
    for row, kind in zip(rows[:2], ("inside", "on")):
        s = s_all[row]; P = d[row] * s[:, None]
        dist = np.linalg.norm(P - L, axis=1); through = through_all[row]
        if kind == "on":
            s = s - np.sqrt(np.maximum(R * R - dist * dist, 0.0)); P = d[row] * s[:, None]
        depth[row] = np.where(through, depth_of(P), depth[row])
        normal[row] = np.where(through[:, None], S.oct_encode(-d[row]), normal[row])
        planted[kind] = (row, int(through.sum()))
    return cam, depth, normal, planted
