"""Which traversal kernels a batch really gets (csrc/walk_plan.hpp: the table next to `enum class Walk`), as the dispatch list of a kernel trace.

Run mode: every situation below that exists as a scene in idkengine_amd/scenes.py renders a batch of 32 samples and a batch of one sample at RayDepth 2 and 5 and makes one
closest-hit and one any-hit idkptTraceRays call.  One process, under the profiler's kernel trace (no counters):

    timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/walk_trace.py

Reduce mode: `python tools/walk_trace.py --reduce DIR > launches.txt` turns the trace into one line per dispatch — kernel, grid, workgroup, LDS bytes as the trace reports them (static LDS only) — under a header that lists the
situations in the order they ran.  Two builds of the library launch the same kernels exactly if their reductions are equal line for line.  Fold mode:
`python tools/walk_trace.py --fold launches.txt` shortens such a reduction to what is kept in the repository (profiles/walk_plan_launches.txt is the shipped library's): one line
per batch or query, holding the dispatches that host_launch.hpp chooses (traversal kernels and the derivations in front of them), equal neighbours counted.  Every batch is waited for before the next is queued, so what the host reads back from the device (previous counts, the packet walk's counters, the instances'
overlap) is the same in every run; where a choice rests on such a measurement the situation additionally pins it with an option, and says so."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 320, 180

# name, scene, options, settings / context switches, what is pinned
SITUATIONS = [
    ("one_blas_packet_forced", "one_blas", dict(packet=2), {}, "packet = 2"),
    ("one_blas_no_packet", "one_blas", dict(packet=0), {}, "packet = 0"),
    ("one_blas_default", "one_blas", {}, {}, ""),
    ("one_blas_counters", "one_blas", dict(packet=2), dict(counters=1), "packet = 2"),
    ("one_blas_use_tlas", "one_blas", dict(packet=2), dict(UseTlas=1), "packet = 2"),
    ("one_blas_debug_view", "one_blas", dict(packet=2), dict(DoDebugBVHTraversal=1), "packet = 2"),
    ("one_blas_two_versions", "one_blas", dict(packet=2), dict(versions=2), "packet = 2"),
    ("one_blas_force_generic", "one_blas", dict(packet=2, force_generic=1), {}, "packet = 2"),
    ("one_blas_wide", "one_blas", dict(packet=0, wide=1), {}, "packet = 0"),
    ("one_blas_wide_packet_forced", "one_blas", dict(packet=2, wide=1, wide_count=1), {}, "packet = 2"),
    ("one_blas_no_last_occlusion", "one_blas", dict(packet=0, last_occlusion=0), {}, "packet = 0"),
    ("one_blas_no_fold_last", "one_blas", dict(packet=0, fold_last=0), {}, "packet = 0"),
    ("one_blas_no_pair_nodes_no_split", "one_blas", dict(packet=0, pair_nodes=0, split=0), {}, "packet = 0"),
    ("one_blas_fused", "one_blas", dict(packet=0, fused=2), {}, "packet = 0"),
    ("one_blas_split_forced", "one_blas", dict(packet=0, split=2), {}, "packet = 0"),
    ("three_rotated", "three_rotated", {}, {}, ""),
    ("three_rotated_general", "three_rotated", dict(inst_general=2), {}, ""),
    ("three_rotated_use_tlas", "three_rotated", {}, dict(UseTlas=1), ""),
    ("twelve_rotated_default", "twelve_rotated", {}, {}, ""),
    ("twelve_rotated_own_tlas", "twelve_rotated", dict(inst_tlas_overlap=100), {}, "inst_tlas_overlap = 100"),
    ("twelve_rotated_sieve", "twelve_rotated", dict(inst_tlas=0, inst_sieve_overlap=100), {}, "inst_sieve_overlap = 100"),
    ("twelve_rotated_loop", "twelve_rotated", dict(inst_tlas=0, inst_sieve=0), {}, ""),
    ("two_same_space_packet_forced", "two_same_space", dict(packet=2), {}, "packet = 2"),
    ("two_same_space_no_packet", "two_same_space", dict(packet=0), {}, "packet = 0"),
    ("two_same_space_no_unify", "two_same_space", dict(packet=2, inst_unify=0), {}, "packet = 2"),
    ("atrium_87_packet_forced", "atrium_87", dict(packet=2), {}, "packet = 2"),
    ("atrium_87_no_packet_refill_16", "atrium_87", dict(packet=0, uni_refill=16), {}, "packet = 0"),
    ("atrium_87_inst_tlas_0_still_unified", "atrium_87", dict(packet=0, inst_tlas=0), {}, "packet = 0"),
    ("atrium_87_no_unify_own_tlas", "atrium_87", dict(packet=2, inst_unify=0, inst_tlas_overlap=100), {}, "packet = 2, inst_tlas_overlap = 100"),
    ("atrium_87_no_unify_sieve", "atrium_87", dict(packet=2, inst_unify=0, inst_tlas=0, inst_sieve_overlap=100), {}, "packet = 2, inst_sieve_overlap = 100"),
    ("rotated_1100_mask_above_rows", "rotated_1100", dict(inst_tlas_overlap=100), {}, "inst_tlas_overlap = 100"),
]


def make_scene(kind):
    from idkengine_amd import scenes as S
    from idkengine_amd.bvh import NativeBuilder
    b = NativeBuilder()
    cam = S.Camera(W, H, position=(1.0, 0.5, 24.0))
    if kind == "one_blas":
        return S.soup_scene(20000, b, seed=5), cam
    if kind == "three_rotated":
        return S.soup_scene_multi(6000, b, parts=3, seed=6), cam
    if kind == "twelve_rotated":
        return S.soup_scene_multi(6000, b, parts=12, seed=15), cam
    if kind == "rotated_1100":
        return S.soup_scene_multi(3300, b, parts=1100, seed=9, extent=4.0, edge=0.4), S.Camera(W, H, position=(0.0, 0.0, 11.0), fovy_deg=60.0)
    if kind == "two_same_space":   # two BLASes, both under the identity: one space
        parts = []
        for k in range(2):
            p, i, nrm, tan = S.flat_shaded(S.soup_triangles(4000, seed=30 + k))
            parts.append({"meshes": [S.MeshInput(p, i, S.make_material((0.8, 0.8, 0.8, 1.0)), nrm, tan)]})
        return S.assemble(parts, b), cam
    return S.atrium_scene(40000, b, per_mesh_blas=True), S.atrium_camera(W, H)


def run():
    from idkengine_amd import scenes as S
    from idkengine_amd.pathtracer import PathTracer
    scenes = {}
    for name, kind, options, switches, _ in SITUATIONS:
        if kind not in scenes:
            scenes[kind] = make_scene(kind)
        sc, cam = scenes[kind]
        pt = PathTracer(W, H)
        pt.set_option("grid_hint", 0)
        for k, v in options.items():
            pt.set_option(k, v)
        if switches.get("versions"):
            pt.SetSceneVersions(switches["versions"])
        if switches.get("counters"):
            pt.enable_counters(True)
        pt.UploadScene(sc); pt.SetCamera(cam)
        for k in ("UseTlas", "DoDebugBVHTraversal"):
            if k in switches:
                setattr(pt, k, switches[k])
        for depth in (2, 5):
            pt.RayDepth = depth
            for batch in (32, 1):
                pt.set_max_batch(batch); pt.ResetAccumulation()
                for _ in range(batch):
                    pt.Compute()
                pt.flush(); pt.synchronize()
        rays = S.primary_ray_queries(cam, W, H)
        pt.TraceRays(rays); pt.TraceRays(rays, any_hit=True)
        pt.synchronize(); pt.Dispose()
        print("done", name, flush=True)


def reduce(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        sys.exit(f"expected one *kernel_trace.csv under {directory}, found {len(files)}")
    rows = list(csv.DictReader(open(files[0], newline="")))
    col = {c.lower(): c for c in rows[0]}
    def pick(*names):
        return next(col[n] for n in names if n in col)
    kid, name, lds = pick("dispatch_id"), pick("kernel_name"), pick("lds_block_size", "lds_block_size_v")   # (the kernel's static LDS: this trace does not carry the dynamic part a launch adds)
    rows.sort(key=lambda r: int(r[kid]))
    print(f"# tools/walk_trace.py: {W} x {H}; per situation RayDepth 2 and 5, each a batch of 32 samples and a batch of one; then one closest-hit and one any-hit idkptTraceRays call.")
    print("# grid_hint = 0 everywhere; every batch is waited for.  Situations in the order they ran (pinned measurement in brackets):")
    for n, kind, options, switches, pinned in SITUATIONS:
        print(f"#   {n}: scene {kind}; {dict(options, **switches) or 'defaults'}" + (f" [{pinned}]" if pinned else ""))
    for r in rows:
        g = "x".join(r[pick(f"grid_size_{a}")] for a in "xyz"); wg = "x".join(r[pick(f"workgroup_size_{a}")] for a in "xyz")
        print(f"{r[name].split('(')[0].replace('void ', '')} grid={g} wg={wg} lds={r[lds]}")


WALK_KERNELS = ("k_trace", "k_packet_mirror", "k_tlas_build", "k_braid", "k_unify_", "k_inst_records", "k_mark_triangles", "k_pair_nodes", "k_wide_")


def counted(items):
    out = []
    for x in items:
        if out and out[-1][1] == x:
            out[-1][0] += 1
        else:
            out.append([1, x])
    return [x if n == 1 else f"{n} x {x}" for n, x in out]


def fold(path):
    lines = [l.rstrip("\n") for l in open(path)]
    print("\n".join(l for l in lines if l.startswith("#")))
    print("# Folded (--fold): one line per batch (ends with k_final_draw) or query (ends with k_query_finish / k_trace_query); of its dispatches those whose kernel host_launch.hpp chooses,")
    print("# as kernel grid/workgroup/LDS bytes (grid in work-items), `n x` = n equal neighbours.  LDS bytes are the kernels' static ones: a kernel trace does not carry the traversal launches' dynamic LDS.  The other stages (generation, shading, scan, compaction, fills and copies) are in the unfolded reduction.")
    names = iter(n for n, *_ in SITUATIONS)
    segs, cur = [], []
    def close(kind):
        nonlocal cur
        if kind or cur:
            segs.append((kind or "setup") + ": " + "; ".join(counted(cur)))
        cur = []
    def flush_segs():
        nonlocal segs
        print("\n".join("  " + x for x in counted(segs))); segs = []
    for l in (l for l in lines if not l.startswith("#")):
        kernel, grid, wg, lds = l.rsplit(" ", 3)
        if kernel == "k_gather_triverts":   # idkptUploadScene: the next situation
            close(""); flush_segs(); print(next(names))
        if kernel.startswith(WALK_KERNELS):
            cur.append(f"{kernel} {grid[5:].split('x')[0]}/{wg[3:].split('x')[0]}/{lds[4:]}")
        if kernel == "k_final_draw":
            close("batch")
        elif kernel == "k_query_finish" or kernel.startswith("k_trace_query"):
            close("query")
    close(""); flush_segs()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--fold":
        sys.exit(fold(sys.argv[2]))
    if len(sys.argv) == 3 and sys.argv[1] == "--reduce":
        reduce(sys.argv[2])
    else:
        run()
