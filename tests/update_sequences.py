"""Random geometry-update sequences (tests/test_update_sequences_ref.py, tests/test_gpu_zy_update_sequences.py): a deterministic generator of host-call sequences over five small
scenes, and a host mirror that applies every op in numpy with the project's restatements (oracle_builder.refit, scenes.rebuild_tlas, plain array writes) and says which C-ABI calls a
context gets for it.  Nothing here imports the library or touches a device.

sequence(seed) is 28 ops: weighted draws (WEIGHTS) with two scripted motifs spliced in per seed (MOTIFS: seed % 7 and (seed + 3) % 7) — four-op transitions such as
xf_all -> compute -> xf_one -> compute do not turn up three times in a dozen seeds by weights alone, and the suite cannot afford the thousands of seeds at which they would."""
import copy
import numpy as np
from idkengine_amd import scenes as S
from idkengine_amd import gputypes as T

LENGTH = 28
DEFAULT_SEEDS = 16
W, H = 96, 64
NAMES = ("a", "b", "c", "d", "e")
# what the generator has to know of a scene without building it (test_update_sequences_ref.py checks the table against the built scenes)
INFO = {"a": dict(instances=1, blases=1, refittable=(0,), materials=1),
        "b": dict(instances=3, blases=3, refittable=(1, 2), materials=3),
        "c": dict(instances=10, blases=10, refittable=(0, 4, 9), materials=10),
        "d": dict(instances=12, blases=12, refittable=(3, 7), materials=12),
        "e": dict(instances=7, blases=2, refittable=(1,), materials=2)}
WEIGHTS = (("compute", 6), ("cam", 2), ("reset", 2), ("depth", 2), ("sort", 2), ("spp", 3), ("batch", 2), ("use_tlas", 2), ("tlas", 2), ("xf_all", 1), ("xf_one", 2), ("xf_range", 3), ("verts", 1),
           ("refit", 1), ("nodes", 1), ("material", 3), ("versions", 1), ("scene", 1), ("query", 2), ("read", 3), ("state", 2))   # (the kinds the motifs bring along weigh half)
KINDS = tuple(k for k, _ in WEIGHTS)
GEOMETRY = ("tlas", "xf_all", "xf_one", "xf_range", "verts", "refit", "nodes", "scene")                      # ops after which the mirror is checked on its own
WALK_CHANGING = ("scene", "xf_all", "xf_one", "xf_range", "verts", "refit", "nodes", "versions", "use_tlas")   # ops after which the library has something to re-derive or another walk to pick
MOTIFS = 7


def cameras(w=W, h=H):
    """far, nearer, and one inside the geometry (a dense view: every ray starts between triangles)"""
    return [S.Camera(w, h, position=(0.5, 0.5, 13.0), fovy_deg=60.0), S.Camera(w, h, position=(-0.4, 0.1, 8.0), fovy_deg=70.0), S.Camera(w, h, position=(0.2, 0.1, 0.3))]


def _soup_blas(n, seed, extent, edge, refittable, transform=None, centre=None):
    tp = S.soup_triangles(n, seed, extent, edge)
    if centre is not None:
        tp = (tp + np.float32(centre)).astype(np.float32)
    p, i, nrm, tan = S.flat_shaded(tp)
    return {"meshes": [S.MeshInput(p, i, S.make_material((0.8, 0.75, 0.7, 1.0)), nrm, tan)], "refittable": refittable, "transform": transform}


def build_scenes(builder):
    """(a) one refittable BLAS; (b) three rotated parts; (c) ten parts on a ring (from the default inst_tlas threshold on); (d) twelve interleaved BLASes under one sheared matrix (the
    unified tree, packets); (e) seven instances of two BLASes, instances 1 and 4 the same BLAS under the same matrix (an exact tie; a BLAS used twice: no unified tree).  Every
    several-BLAS scene has a refittable BLAS with BlasId > 0.  (b) and (c) are scenes.soup_scene_multi's layout restated on scenes.assemble: that function cannot mark single parts
    refittable, and (c)'s parts sit on a ring so that their boxes overlap little.)"""
    sc = {}
    sc["a"] = S.soup_scene(3000, builder, seed=31, refittable=True, extent=2.5, edge=0.3)
    sc["b"] = S.assemble([_soup_blas(1000, 40 + 17 * k, 2.5, 0.3, k in INFO["b"]["refittable"], None if k == 0 else S.rotation_y(23.0 * k) @ S.translation((0.5 * k, -0.25 * k, 0.0))) for k in range(3)], builder)
    ring = [(4.0 * np.cos(2 * np.pi * k / 10), 4.0 * np.sin(2 * np.pi * k / 10), 0.4 * (k % 3)) for k in range(10)]
    sc["c"] = S.assemble([_soup_blas(400, 60 + 17 * k, 1.1, 0.3, k in INFO["c"]["refittable"], None if k == 0 else S.rotation_y(23.0 * k), centre=ring[k]) for k in range(10)], builder)
    sh = np.eye(4); sh[0, 1] = 0.35; sh[2, 0] = -0.2
    m = S.rotation_y(33.0) @ np.diag([1.3, 0.8, 1.1, 1.0]) @ sh @ S.translation((0.5, -0.25, 1.0))
    sc["d"] = S.assemble([_soup_blas(300, 80 + 17 * k, 3.0, 0.35, k in INFO["d"]["refittable"], m) for k in range(12)], builder)
    e = S.assemble([_soup_blas(1500, 5 + 31 * k, 3.0, 0.3, k in INFO["e"]["refittable"]) for k in range(2)], builder, build_tlas=False)
    em = [np.eye(4), S.rotation_y(30.0) @ S.translation((2.0, 0.0, 0.0)), S.rotation_y(-50.0) @ S.translation((-2.5, 0.5, 1.0)), S.translation((0.0, 3.0, -2.0)),
          S.rotation_y(30.0) @ S.translation((2.0, 0.0, 0.0)), S.rotation_y(75.0) @ S.translation((1.0, -3.0, 0.0)), S.rotation_y(-50.0) @ S.translation((-2.5, 0.5 + 1e-6, 1.0))]
    inst = np.zeros(7, T.GpuBlasInstance); inst["BlasId"] = [0, 1, 0, 1, 1, 0, 0]; inst["MeshTransformId"] = np.arange(7)
    e.blas_instances = inst; e.mesh_transforms = np.concatenate([S.transform_from_matrix(x) for x in em])
    S.rebuild_tlas(e, builder)
    sc["e"] = e
    return sc


# ---- matrices ------------------------------------------------------------------------------------------------------------------------------------------------------
def _draw_matrix(rng, zero_ok=False):
    if zero_ok and rng.integers(0, 20) == 0:
        return ("zero",)
    t = tuple(round(float(x), 3) for x in rng.uniform(-2.0, 2.0, 3))
    k = int(rng.integers(0, 3))
    if k == 0:
        return ("rigid", round(float(rng.uniform(0.0, 360.0)), 2), t)
    if k == 1:
        return ("scale", tuple(round(float(x), 3) for x in rng.uniform(0.5, 1.6, 3)), t)
    return ("shear", tuple(round(float(x), 3) for x in rng.uniform(-0.4, 0.4, 2)), t)


def transform(spec):
    """GpuMeshTransform[1] of a matrix spec; "zero": an instance hidden by a zero scale (Model = InvModel = 0)."""
    if spec[0] == "zero":
        return np.zeros(1, T.GpuMeshTransform)
    if spec[0] == "rigid":
        m = S.rotation_y(spec[1])
    elif spec[0] == "scale":
        m = np.diag([spec[1][0], spec[1][1], spec[1][2], 1.0])
    else:
        m = np.eye(4); m[0, 1] = spec[1][0]; m[2, 0] = spec[1][1]
    return S.transform_from_matrix(m @ S.translation(spec[2]))


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, scene):
        self.scene, self.use_tlas, self.versions = scene, 0, 1


def _op(kind, g, rng):
    info = INFO[g.scene]
    if kind in ("compute", "reset", "tlas", "read", "state"):
        return (kind,)
    if kind == "cam":
        return (kind, int(rng.integers(0, 3)))
    if kind == "depth":
        return (kind, int(rng.integers(1, 6)))
    if kind == "sort":
        return (kind, int(rng.integers(0, 2)))
    if kind == "spp":
        return (kind, int(rng.integers(1, 4)))
    if kind == "batch":
        return (kind, int(rng.integers(1, 9)))
    if kind == "use_tlas":
        g.use_tlas ^= 1
        return (kind, g.use_tlas)
    if kind == "xf_all":
        return (kind, _draw_matrix(rng))
    if kind == "xf_one":
        return (kind, int(rng.integers(0, info["instances"])), _draw_matrix(rng, zero_ok=True))
    if kind == "xf_range":
        n = int(rng.integers(1, min(3, info["instances"]) + 1)); first = int(rng.integers(0, info["instances"] - n + 1))
        return (kind, first, tuple(_draw_matrix(rng) for _ in range(n)))
    if kind == "verts":
        return (kind, int(rng.integers(0, info["blases"])), int(rng.integers(2, 9)), int(rng.integers(0, 1 << 30)))
    if kind == "refit":
        return (kind, int(rng.choice(info["refittable"])))
    if kind == "nodes":
        return (kind, int(rng.integers(0, info["blases"])))
    if kind == "material":
        return (kind, int(rng.integers(0, info["materials"])), tuple(round(float(x), 3) for x in rng.uniform(0.0, 0.5, 3)))
    if kind == "versions":
        g.versions = int(rng.choice([1, 1, 3]))
        return (kind, g.versions)
    if kind == "scene":
        others = [n for n in NAMES if n != g.scene]      # another scene than the one loaded (the motifs may re-upload the same one)
        g.scene = others[int(rng.integers(0, len(others)))]
        return (kind, g.scene)
    if kind == "query":
        return (kind, int(rng.integers(0, 1 << 30)))
    raise ValueError(kind)


def _motif(which, g, rng):
    """The transitions test_update_sequences_ref.py asks for, each as a contiguous run (a scene with several BLASes first where the run needs one)."""
    out = []
    def to_scene(names):
        if g.scene not in names:
            g.scene = names[int(rng.integers(0, len(names)))]; out.append(("scene", g.scene))
    def refittable_beyond_zero():
        return int(rng.choice([b for b in INFO[g.scene]["refittable"] if b > 0]))
    if which == 0:                                        # one space, then out of it
        to_scene(("b", "c", "d")); out += [_op("xf_all", g, rng), ("compute",), _op("xf_one", g, rng), ("compute",)]
    elif which == 1:                                      # ... and back into one space
        to_scene(("b", "c", "d")); out += [_op("xf_one", g, rng), ("compute",), _op("xf_all", g, rng), ("compute",)]
    elif which == 2:                                      # a tree derived at one version, three versions, an update in flight, back to one
        to_scene(("c", "d")); g.versions = 1
        if g.use_tlas:                                    # (the optional walks, and the loop at three versions, are walks without UseTlas)
            g.use_tlas = 0; out.append(("use_tlas", 0))
        out += [("versions", 1), ("compute",), ("versions", 3), _op("xf_all", g, rng), ("compute",), ("versions", 1), ("compute",)]
    elif which == 3:                                      # many instances -> one -> many
        big = ("c", "d")[int(rng.integers(0, 2))]; g.scene = big
        out += [("scene", big), ("compute",), ("scene", "a"), ("compute",), ("scene", big), ("compute",)]
    elif which == 4:                                      # k_refit_* with non-zero node / triangle offsets
        to_scene(("b", "c", "d", "e")); b = refittable_beyond_zero()
        out += [("verts", b, int(rng.integers(2, 9)), int(rng.integers(0, 1 << 30))), ("refit", b), ("compute",)]
    elif which == 5:                                      # stale boxes seen, then refitted ones
        to_scene(("b", "c", "d", "e")); b = refittable_beyond_zero()
        out += [("verts", b, int(rng.integers(2, 9)), int(rng.integers(0, 1 << 30))), ("compute",), ("refit", b), ("compute",)]
    else:                                                 # the same state by the other door
        to_scene(("b", "c", "d", "e")); b = int(rng.integers(1, INFO[g.scene]["blases"]))
        out += [("verts", b, int(rng.integers(2, 9)), int(rng.integers(0, 1 << 30))), ("nodes", b), ("compute",)]
    return out


def sequence(seed):
    rng = np.random.default_rng(7000 + int(seed))
    g = _Gen(NAMES[seed % len(NAMES)])
    motifs = [(seed % MOTIFS, int(rng.integers(2, 6))), ((seed + 3) % MOTIFS, int(rng.integers(15, 19)))]
    kinds = np.array(KINDS); p = np.array([w for _, w in WEIGHTS], np.float64); p /= p.sum()
    ops = []
    while len(ops) < LENGTH:
        if motifs and len(ops) >= motifs[0][1]:
            ops += _motif(motifs.pop(0)[0], g, rng)
            continue
        ops.append(_op(str(rng.choice(kinds, p=p)), g, rng))
    assert len(ops) == LENGTH, len(ops)
    return ops


def start_scene(seed):
    return NAMES[seed % len(NAMES)]


def query_rays(qseed, n=512, short=64):
    """n closest-hit queries from a fixed generator: origins in the scenes' extent, the first `short` of them with a maximal distance that ends most of them before their hit."""
    rng = np.random.default_rng(qseed)
    r = np.zeros(n, T.RayQuery)
    r["Origin"] = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    r["Direction"] = d.astype(np.float32); r["MaxDist"] = np.float32(3.4028235e+38); r["MaxDist"][:short] = np.float32(1.5)
    return r


# ---- the host mirror -------------------------------------------------------------------------------------------------------------------------------------------------
class Mirror:
    """The scene as the host believes the device holds it, and the settings a frame is rendered with.  apply(op) changes it and returns the calls a context gets for the op:
    tuples (method name of PathTracer, *arguments); "attr" sets a property, "camera" takes an index into cameras()."""

    def __init__(self, scenes, name, oracle_builder):
        self.scenes, self.ob = scenes, oracle_builder
        self.settings = dict(RayDepth=3, DoRaySorting=0, SamplesPerPixel=1, UseTlas=0)
        self.cam, self.versions = 0, 1
        self._load(name)

    def _load(self, name):
        self.name = name; self.scene = copy.deepcopy(self.scenes[name]); self.tlas_built = False; self.tlas_fresh = True

    def _slices(self, b):
        d = self.scene.blas_descs[b]
        return slice(int(d["NodeOffset"]), int(d["NodeOffset"] + d["NodeCount"])), slice(int(d["TriangleOffset"]), int(d["TriangleOffset"] + d["TriangleCount"]))

    def _refit(self, b):
        ns, ts = self._slices(b)
        self.scene.blas_nodes[ns] = self.ob.refit(self.scene.blas_nodes[ns], self.scene.vertex_positions, self.scene.blas_triangles[ts])
        return ns

    def apply(self, op):
        k, sc = op[0], self.scene
        xb = T.GpuMeshTransform.itemsize
        if k == "compute":
            return [("Compute",)]
        if k == "reset":
            return [("ResetAccumulation",)]
        if k == "cam":
            self.cam = op[1]; return [("camera", op[1])]
        if k in ("depth", "sort", "spp", "use_tlas"):
            name = {"depth": "RayDepth", "sort": "DoRaySorting", "spp": "SamplesPerPixel", "use_tlas": "UseTlas"}[k]
            self.settings[name] = op[1]; return [("attr", name, op[1])]
        if k == "batch":
            return [("set_max_batch", op[1])]
        if k == "versions":
            self.versions = op[1]; return [("SetSceneVersions", op[1])]
        if k == "tlas":
            S.rebuild_tlas(sc, self.ob); self.tlas_built = True; self.tlas_fresh = True
            return [("BuildTlasOnDevice",)]
        if k == "scene":
            self._load(op[1]); return [("UploadScene", self.scene)]
        self.tlas_fresh = self.tlas_fresh and k in ("material", "query", "read", "state")     # (verts alone moves no box, but a later refit does: the flag only ever says "certainly fresh")
        if k == "xf_all":
            xf = np.repeat(transform(op[1]), len(sc.mesh_transforms)); sc.mesh_transforms = xf
            return [("UpdateBuffer", T.IDKPT_BUF_MESH_TRANSFORMS, xf.copy(), 0)]
        if k == "xf_one":
            i = int(sc.blas_instances["MeshTransformId"][op[1]]); sc.mesh_transforms[i] = transform(op[2])[0]
            return [("UpdateBuffer", T.IDKPT_BUF_MESH_TRANSFORMS, sc.mesh_transforms[i:i + 1].copy(), i * xb)]
        if k == "xf_range":
            sub = np.concatenate([transform(m) for m in op[2]]); sc.mesh_transforms[op[1]:op[1] + len(sub)] = sub
            return [("UpdateBuffer", T.IDKPT_BUF_MESH_TRANSFORMS, sub, op[1] * xb)]
        if k == "verts":
            _, ts = self._slices(op[1]); t = sc.blas_triangles[ts]
            ids = np.unique(np.concatenate([t["X"], t["Y"], t["Z"]]))[::op[2]]
            sc.vertex_positions[ids] += np.random.default_rng(op[3]).uniform(-0.05, 0.05, (len(ids), 3)).astype(np.float32)
            return [("UpdateBuffer", T.IDKPT_BUF_VERTEX_POSITIONS, sc.vertex_positions.copy(), 0)]
        if k == "refit":
            self._refit(op[1]); return [("RefitBlas", op[1])]
        if k == "nodes":
            ns = self._refit(op[1])
            return [("UpdateBuffer", T.IDKPT_BUF_BLAS_NODES, sc.blas_nodes[ns].copy(), ns.start * T.GpuBlasNode.itemsize)]
        if k == "material":
            sc.materials["EmissiveFactor"][op[1]] = op[2]
            return [("UpdateBuffer", T.IDKPT_BUF_MATERIALS, sc.materials[op[1]:op[1] + 1].copy(), op[1] * T.GpuMaterial.itemsize)]
        if k in ("query", "read", "state"):
            return []
        raise ValueError(k)

    # what the oracle says of the mirror
    def oracle_frame(self, O, w=W, h=H):
        o = O.OraclePathTracer(self.scene, w, h); o.set_camera(cameras(w, h)[self.cam])
        for name, v in self.settings.items():
            setattr(o.settings, name, v)
        o.render()
        return o

    def oracle_hits(self, O, rays):
        return O.trace_rays(self.scene, rays, use_tlas=bool(self.settings["UseTlas"]))


def play(pt, calls, cams, product=True):
    """Hands `calls` (Mirror.apply) to a PathTracer.  product = False: the plain replay, which keeps max batch 1 and one scene version."""
    for c in calls:
        if c[0] == "attr":
            setattr(pt, c[1], c[2])
        elif c[0] == "camera":
            pt.SetCamera(cams[c[1]])
        elif c[0] in ("set_max_batch", "SetSceneVersions"):
            if product:
                getattr(pt, c[0])(c[1])
        else:
            getattr(pt, c[0])(*c[1:])
