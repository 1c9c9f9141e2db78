"""Which traversal walk a batch gets (idkengine_amd/csrc/walk_plan.hpp: choose_walk, packet_vote / packet_primary), situation by situation.  The header is pure C++ — no HIP, no
context — so g++ compiles it into a small program here.  The expectations were written from the dispatch logic as it stood before the decision was gathered into that header and
are backed by the kernel trace of the same situations on the device (profiles/walk_plan_launches.txt, tools/walk_trace.py); they are not read off choose_walk.

A situation names the scene shape and the options; what the device would report (inst_tlas_derive: the unified tree, whether a tree / the sieve is worth it) is modelled from three facts
about the scene: are the instances one space, do their boxes overlap little enough for the own TLAS (inst_tlas_overlap), for the sieve (inst_sieve_overlap)."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r"""
#include "walk_plan.hpp"
#include <stdio.h>
#include <string.h>
using namespace walk;
static const char* NAMES[] = {"Generic", "Plain", "Fast", "Loop", "Tlas", "Wide", "OwnTlas", "Unified", "General", "Sieve"};
struct Facts { bool sameSpace = false, treeOverlapOk = false, sieveOverlapOk = false, packetMeasuredOn = true, fused = false; int instGeneral = 0, tlasDepth = 0; };
static WalkInputs defaults()
{
    WalkInputs in; memset(&in, 0, sizeof(in));
    in.instanceCount = 1; in.verSlots = 1; in.sceneNested = true;
    in.pairNodes = 1; in.packet = 1; in.instTlas = 8; in.instSieve = 8; in.instUnify = 4096; in.queryScheduler = true;
    in.pixelMajor = true;   // a batch of 32 samples
    return in;
}
// what inst_tlas_derive leaves in the context for this scene (host_launch.hpp), and the LDS rows behind the BLAS stack (inst_tlas_rows)
static void derive(WalkInputs& in, const Facts& f)
{
    const bool gate = in.query ? (in.queryScheduler && !in.debugView && !in.anyHit && in.instanceCount > 1 && !in.useTlas) : fast_path(in);
    const bool wantU = inst_unify_wanted(in), wantS = inst_tlas_wanted(in, true);
    if (gate && (wantU || inst_tlas_wanted(in) || wantS)) {
        in.uniMode = wantU ? unify_mode(f.sameSpace, in.instanceCount, f.instGeneral) : 0; in.uniValid = in.uniMode != 0;
        in.itlasBuilt = in.uniValid || (inst_tlas_wanted(in) && f.treeOverlapOk);
        in.isieveWorth = !in.itlasBuilt && wantS && f.sieveOverlapOk;
        in.itlasValid = true;
    }
    in.maskWords = (in.instanceCount + 31) / 32;
    in.maskRows = in.itlasBuilt && f.tlasDepth > 0 ? std::min(32, std::max(in.maskWords, f.tlasDepth)) : std::min(32, std::max(1, in.instanceCount));
}
static void report(const char* name, WalkInputs in, const Facts& f)
{
    derive(in, f);
    const Walk w = choose_walk(in);
    const PacketVote v = packet_vote(in);
    const bool packetBatch = !in.query && fast_path(in) && !in.multiVer && !in.useTlas && (v == PacketVote::Yes || (v == PacketVote::Measure && f.packetMeasuredOn)) && !f.fused;
    printf("%s %s %d %d %d\n", name, NAMES[(int)w], packet_primary(in, w, packetBatch) ? 1 : 0, in.maskWords <= in.maskRows ? 1 : 0, split_allowed(in, w) ? 1 : 0);
}
int main()
{
    SITUATIONS
    return 0;
}
"""

# the scene shapes: instance count and the three facts
ONE = dict(n=1)
ROT3 = dict(n=3)                                                  # three instances under different transforms
ROT12_APART = dict(n=12, treeOverlapOk=1, sieveOverlapOk=1)       # twelve, boxes that overlap little
ROT12_DENSE = dict(n=12, sieveOverlapOk=1)                        # ... too much for the own TLAS, not for the sieve
ROT12_SOUP = dict(n=12)                                           # ... too much for both
SAME2 = dict(n=2, sameSpace=1)
SAME87 = dict(n=87, sameSpace=1, treeOverlapOk=1, sieveOverlapOk=1, tlasDepth=9)
ROT1500 = dict(n=1500, treeOverlapOk=1, sieveOverlapOk=1, tlasDepth=14)
ROT5000 = dict(n=5000, treeOverlapOk=1, sieveOverlapOk=1)

# name: (scene, inputs that differ from the defaults, (walk, packet walk on the primary launch of bounce 0))
FRAMES = {
    "one_blas_default": (ONE, {}, ("Fast", 1)),
    "one_blas_one_sample": (ONE, dict(pixelMajor=0), ("Fast", 0)),                       # tile-major list: packet = 1 does not ask
    "one_blas_packet_measured_off": (ONE, dict(packetMeasuredOn=0), ("Fast", 0)),
    "one_blas_fused": (ONE, dict(fused=1), ("Fast", 0)),
    "one_blas_counters": (ONE, dict(counters=1), ("Plain", 0)),
    "one_blas_use_tlas": (ONE, dict(useTlas=1), ("Tlas", 0)),
    "one_blas_debug_view": (ONE, dict(debugView=1), ("Generic", 0)),
    "one_blas_two_versions_in_the_batch": (ONE, dict(verSlots=2, multiVer=1), ("Plain", 0)),
    "one_blas_two_versions_allowed": (ONE, dict(verSlots=2), ("Plain", 0)),
    "one_blas_force_generic": (ONE, dict(forceGeneric=1), ("Generic", 0)),
    "one_blas_wide": (ONE, dict(wide=1), ("Wide", 1)),                                   # the packet walk takes the primary launch, the wide-node walk the bounces
    "one_blas_wide_variant_213": (ONE, dict(wide=1, traceVariant=213), ("Wide", 0)),
    "one_blas_wide_counters": (ONE, dict(wide=1, counters=1), ("Plain", 0)),
    "one_blas_variant_213": (ONE, dict(traceVariant=213), ("Plain", 0)),
    "one_blas_no_pair_nodes": (ONE, dict(pairNodes=0), ("Plain", 1)),
    "one_blas_packet_0": (ONE, dict(packet=0), ("Fast", 0)),
    "one_blas_packet_2": (ONE, dict(packet=2, pixelMajor=0, packetMeasuredOn=0), ("Fast", 1)),
    "one_blas_packet_2_not_nested": (ONE, dict(packet=2, sceneNested=0), ("Fast", 0)),
    "three_rotated": (ROT3, {}, ("Loop", 0)),
    "three_rotated_inst_general_2": (ROT3, dict(instGeneral=2), ("General", 0)),
    "three_rotated_use_tlas": (ROT3, dict(useTlas=1), ("Tlas", 0)),
    "three_rotated_counters": (ROT3, dict(counters=1, instGeneral=2), ("Loop", 0)),
    "twelve_apart": (ROT12_APART, {}, ("OwnTlas", 0)),
    "twelve_dense": (ROT12_DENSE, {}, ("Sieve", 0)),
    "twelve_soup": (ROT12_SOUP, {}, ("Loop", 0)),
    "twelve_apart_inst_tlas_0": (ROT12_APART, dict(instTlas=0), ("Sieve", 0)),
    "twelve_apart_inst_tlas_0_inst_sieve_0": (ROT12_APART, dict(instTlas=0, instSieve=0), ("Loop", 0)),
    "twelve_apart_force_generic": (ROT12_APART, dict(forceGeneric=1), ("Generic", 0)),
    "two_same_space": (SAME2, {}, ("Unified", 1)),
    "two_same_space_packet_0": (SAME2, dict(packet=0), ("Unified", 0)),
    "two_same_space_inst_unify_0": (SAME2, dict(instUnify=0, packet=2), ("Loop", 0)),
    "two_same_space_not_nested": (SAME2, dict(sceneNested=0, packet=2), ("Loop", 0)),
    "same_space_87": (SAME87, {}, ("Unified", 1)),
    "same_space_87_one_sample": (SAME87, dict(pixelMajor=0), ("Unified", 0)),
    "same_space_87_inst_unify_0": (SAME87, dict(instUnify=0, packet=2), ("OwnTlas", 0)),
    "same_space_87_inst_tlas_0": (SAME87, dict(instTlas=0), ("Unified", 1)),              # inst_tlas = 0 does not turn the unified tree off
    "same_space_87_inst_tlas_0_inst_unify_0": (SAME87, dict(instTlas=0, instUnify=0), ("Sieve", 0)),
    "same_space_87_use_tlas": (SAME87, dict(useTlas=1), ("Tlas", 0)),
    "rotated_1500": (ROT1500, {}, ("OwnTlas", 0)),                                        # more than 1024: no sieve, no unified tree
    "same_space_1500": (dict(ROT1500, sameSpace=1), {}, ("OwnTlas", 0)),
    "rotated_1500_dense": (dict(ROT1500, treeOverlapOk=0), {}, ("Loop", 0)),
    "rotated_5000": (ROT5000, {}, ("Loop", 0)),                                           # more than 4096: the loop
}
# closest hit, any hit
QUERIES = {
    "query_one_blas": (ONE, {}, ("Plain", "Plain")),
    "query_one_blas_use_tlas": (ONE, dict(useTlas=1), ("Tlas", "Tlas")),
    "query_one_blas_debug_view": (ONE, dict(debugView=1), ("Generic", "Generic")),
    "query_one_blas_no_scheduler": (ONE, dict(queryScheduler=0), ("Generic", "Generic")),
    "query_three_rotated": (ROT3, {}, ("Loop", "Loop")),
    "query_three_rotated_inst_general_2": (ROT3, dict(instGeneral=2), ("Sieve", "Loop")),
    "query_twelve_apart": (ROT12_APART, {}, ("Sieve", "Loop")),
    "query_twelve_dense": (ROT12_DENSE, {}, ("Sieve", "Loop")),
    "query_twelve_soup": (ROT12_SOUP, {}, ("Loop", "Loop")),
    "query_twelve_apart_force_generic": (ROT12_APART, dict(forceGeneric=1), ("Sieve", "Loop")),   # force_generic is about frames
    "query_two_same_space": (SAME2, {}, ("Sieve", "Loop")),
    "query_same_space_87": (SAME87, {}, ("Sieve", "Loop")),
    "query_same_space_87_use_tlas": (SAME87, dict(useTlas=1), ("Tlas", "Tlas")),
    "query_rotated_1500": (ROT1500, {}, ("Sieve", "Loop")),
    "query_rotated_5000": (ROT5000, {}, ("Loop", "Loop")),
}
FACTS = ("sameSpace", "treeOverlapOk", "sieveOverlapOk", "packetMeasuredOn", "fused", "instGeneral", "tlasDepth")


def _block(name, scene, inputs, **more):
    kv = dict(scene, **inputs, **more)
    lines = ["{ WalkInputs in = defaults(); Facts f;", f"in.instanceCount = {kv.pop('n')};"]
    lines += [f"{'f' if k in FACTS else 'in'}.{k} = {int(v)};" for k, v in kv.items()]
    return " ".join(lines) + f' report("{name}", in, f); }}'


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_plan")
    blocks = [_block(n, sc, inp) for n, (sc, inp, _) in FRAMES.items()]
    for n, (sc, inp, _) in QUERIES.items():
        blocks += [_block(n + ":closest", sc, inp, query=1), _block(n + ":any", sc, inp, query=1, anyHit=1)]
    src = d / "walk_plan_test.cpp"; src.write_text(HARNESS.replace("SITUATIONS", "\n    ".join(blocks)))
    exe = d / "walk_plan_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "idkengine_amd", "csrc"), str(src), "-o", str(exe)])   # (no HIP anywhere on the include path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {l.split()[0]: l.split()[1:] for l in out.splitlines()}


@pytest.mark.parametrize("name", list(FRAMES))
def test_frames(answers, name):
    walk, packet = FRAMES[name][2]
    assert (answers[name][0], int(answers[name][1])) == (walk, packet)


@pytest.mark.parametrize("name", list(QUERIES))
def test_queries(answers, name):
    closest, any_hit = QUERIES[name][2]
    assert (answers[name + ":closest"][0], answers[name + ":any"][0]) == (closest, any_hit)
    assert answers[name + ":closest"][1] == "0" and answers[name + ":any"][1] == "0"      # no packets for queries


def test_flagged_rays_and_the_split(answers):
    # a lane's mask of 1500 instances has 47 words, LDS has 32 rows for it: the flagged rays go to k_trace2 MODE 1 instead of the sieved loop
    assert answers["rotated_1500"][2] == "0" and answers["same_space_87"][2] == "1" and answers["twelve_apart"][2] == "1"
    # k_trace2s stands in for Plain / Fast only: one version, no counters, boxes that nest
    assert answers["one_blas_default"][3] == "1" and answers["one_blas_no_pair_nodes"][3] == "1"
    for n in ("one_blas_counters", "one_blas_two_versions_in_the_batch", "one_blas_wide", "one_blas_use_tlas", "three_rotated", "same_space_87", "one_blas_packet_2_not_nested", "one_blas_variant_213"):
        assert answers[n][3] == "0", n
