"""Which write makes which derived scene structure stale (idkengine_amd/csrc/derived_scene.hpp: stale_after, stale_with, State).  The header is pure C++ — no HIP, no context — so
g++ compiles it into a small program here, as tests/test_walk_plan.py does with its header.  The sets below are written out from the rule as it stood when it was spread over
ver_reset, ver_invalidate, the BLAS-node patch of idkptUpdateBuffer and the inst_* options (DESIGN.md "Derived scene structures" has the same table); they are not read off the header.
The device side of the same promise: tests/test_gpu_derived_scene.py, tests/test_gpu_zy_update_sequences.py."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTURES = ("PAIR", "WIDE_TOPO", "WIDE_FILL", "INST_REC", "MARKS", "CHUNKS", "OWN_TLAS", "OVERLAP_KNOWN", "TLAS_BUILT", "UNI", "UNI_TABS")
CAUSES = ("SceneReplaced", "NodesPatched", "WriteNodes", "WriteTriVerts", "WriteVertices", "WriteTlas", "WriteXforms", "InstOption")
STALE = {
    "SceneReplaced": set(STRUCTURES),
    "NodesPatched": {"PAIR", "WIDE_TOPO", "WIDE_FILL", "OWN_TLAS", "INST_REC", "MARKS"},
    "WriteNodes": {"PAIR", "WIDE_FILL", "MARKS", "OWN_TLAS", "INST_REC"},
    "WriteTriVerts": {"WIDE_FILL", "MARKS"},
    "WriteVertices": set(),
    "WriteTlas": set(),
    "WriteXforms": {"OWN_TLAS", "INST_REC"},
    "InstOption": {"OWN_TLAS"},
}
HANGS_UNDER = {"OWN_TLAS": {"UNI"}, "WIDE_TOPO": {"WIDE_FILL"}}   # deriving the key anew makes these stale; nothing hangs under any other structure

HARNESS = r"""
#include "derived_scene.hpp"
#include <stdio.h>
using namespace derived;
static const Structure S[] = {%(structures)s};
static const char* SN[] = {%(structure_names)s};
static const Cause C[] = {%(causes)s};
static const char* CN[] = {%(cause_names)s};
static void names(uint32_t bits) { for (int i = 0; i < %(ns)d; i++) if (bits & S[i]) printf(" %%s", SN[i]); printf("\n"); }
static_assert(stale_after(Cause::WriteVertices) == 0u && stale_after(Cause::WriteTlas) == 0u, "the table is a constant expression");
int main()
{
    uint32_t all = 0; for (int i = 0; i < %(ns)d; i++) { if (all & S[i]) return 1; all |= S[i]; }      // eleven different bits
    printf("bits %%d %%d\n", __builtin_popcount(all), all == (uint32_t)ALL ? 1 : 0);
    for (int c = 0; c < %(nc)d; c++) {
        printf("stale %%s", CN[c]); names(stale_after(C[c]));
        State st; for (int i = 0; i < %(ns)d; i++) st.mark(S[i]);                                         // everything derived, the packet decision made
        st.pkState = 2; st.pkBatchesSinceProbe = 7;
        st.invalidate(C[c]);
        printf("left %%s", CN[c]); names(st.valid);
        printf("extra %%s %%d\n", CN[c], (st.valid & ~all) ? 1 : 0);
        printf("packet %%s %%d %%d\n", CN[c], st.pkState, st.pkBatchesSinceProbe);
        State none; none.invalidate(C[c]); printf("fromnone %%s %%u\n", CN[c], none.valid);
    }
    for (int i = 0; i < %(ns)d; i++) {
        printf("with %%s", SN[i]); names(stale_with(S[i]));
        State st; for (int k = 0; k < %(ns)d; k++) st.mark(S[k]);
        st.rederiving(S[i]);
        printf("rederiving %%s", SN[i]); names(st.valid);
        State one; one.mark(S[i]);
        printf("holds %%s", SN[i]); for (int k = 0; k < %(ns)d; k++) if (one.holds(S[k])) printf(" %%s", SN[k]); printf("\n");
        one.mark(S[i], false); printf("unmarked %%s %%u\n", SN[i], one.valid);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("derived_scene")
    src = d / "derived_scene_test.cpp"
    src.write_text(HARNESS % dict(structures=", ".join(STRUCTURES), structure_names=", ".join(f'"{s}"' for s in STRUCTURES), ns=len(STRUCTURES),
                                  causes=", ".join("Cause::" + c for c in CAUSES), cause_names=", ".join(f'"{c}"' for c in CAUSES), nc=len(CAUSES)))
    exe = d / "derived_scene_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "idkengine_amd", "csrc"), str(src), "-o", str(exe)])   # (no HIP anywhere on the include path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    return {tuple(l.split()[:2]): l.split()[2:] for l in out.splitlines()}


def test_eleven_structures_one_bit_each(answers):
    assert answers[("bits", "11")] == ["1"]


@pytest.mark.parametrize("cause", CAUSES)
def test_what_goes_stale(answers, cause):
    assert set(answers[("stale", cause)]) == STALE[cause]
    assert len(answers[("stale", cause)]) == len(STALE[cause])


@pytest.mark.parametrize("cause", CAUSES)
def test_invalidate_after_marking_everything_leaves_the_complement(answers, cause):
    assert set(answers[("left", cause)]) == set(STRUCTURES) - STALE[cause]
    assert answers[("extra", cause)] == ["0"] and answers[("fromnone", cause)] == ["0"]       # no bit beyond the eleven, nothing set by an invalidation


def test_vertices_and_host_tlas_clear_nothing(answers):
    for cause in ("WriteVertices", "WriteTlas"):
        assert answers[("stale", cause)] == [] and set(answers[("left", cause)]) == set(STRUCTURES)


def test_only_a_replaced_scene_restarts_the_packet_probe(answers):
    for cause in CAUSES:
        assert answers[("packet", cause)] == (["0", "0"] if cause == "SceneReplaced" else ["2", "7"]), cause


@pytest.mark.parametrize("structure", STRUCTURES)
def test_dependencies(answers, structure):
    under = HANGS_UNDER.get(structure, set())
    assert set(answers[("with", structure)]) == under
    assert set(answers[("rederiving", structure)]) == set(STRUCTURES) - under                 # the structure itself stays as it was: its derivation marks it
    assert answers[("holds", structure)] == [structure] and answers[("unmarked", structure)] == ["0"]
