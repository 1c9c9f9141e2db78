// derived_scene.hpp — what the library derives on the device from what the host uploads, and which write makes which of it stale: the rule as data.  Nothing from HIP and no
// dev_ctx in here: g++ compiles this header on its own (tests/test_derived_scene.py).  The owner of the buffers — DerivedScene, host_context.hpp — builds on State below; the
// derivations (*_prepare, host_derived.hpp) run lazily in front of the batch that needs them and mark what they made.  DESIGN.md "Derived scene structures" has the table in words.
#pragma once
#include <stdint.h>
namespace derived {
// one bit per structure (State::valid)
enum Structure : uint32_t {
    PAIR = 1u << 0,            // the paired node layout (k_pair_nodes; k_trace2 FAST)
    WIDE_TOPO = 1u << 1,       // the 4-wide nodes' children lists (k_wide_topo)
    WIDE_FILL = 1u << 2,       // ... their boxes and leaf records (k_wide_fill)
    INST_REC = 1u << 3,        // the instance records (k_inst_records)
    MARKS = 1u << 4,           // the per-triangle marks "not contained in its leaf box" (k_mark_triangles)
    CHUNKS = 1u << 5,          // the (BLAS, chunk of 256 nodes) table
    OWN_TLAS = 1u << 6,        // the library's own TLAS with its braid entries, and every measured decision that rides on it (tree worth it, sieve worth it, depth, entries)
    OVERLAP_KNOWN = 1u << 7,   // the instances' overlap has been read at least once since the upload (later measurements are not waited for)
    TLAS_BUILT = 1u << 8,      // the last measurement said the tree is worth it, and it was built
    UNI = 1u << 9,             // the unified tree / the general array
    UNI_TABS = 1u << 10,       // ... its per-BLAS tables, and whether the scene is eligible for it at all
    ALL = (1u << 11) - 1u
};
// what the host does to the scene
enum class Cause {
    SceneReplaced,             // idkptUploadScene, a clone, a re-derived node order: every caller of ver_reset
    NodesPatched,              // idkptUpdateBuffer of BLAS nodes: the tree itself may have changed
    WriteNodes, WriteTriVerts, WriteVertices, WriteTlas, WriteXforms,   // a versioned buffer is about to be written (ver_writable), in VB_* order
    InstOption                 // one of the inst_* options: what is wanted of the own TLAS changed
};
// THE table: what goes stale.  (Node boxes or triangle positions move: the wide nodes' boxes and leaf records and the triangle marks; root boxes or transforms move: the own TLAS and
// the instance records; a patched tree additionally changes the children lists.  The vertices and the host's TLAS feed nothing derived.)
constexpr uint32_t stale_after(Cause c)
{
    return c == Cause::SceneReplaced ? (uint32_t)ALL
         : c == Cause::NodesPatched  ? PAIR | WIDE_TOPO | WIDE_FILL | OWN_TLAS | INST_REC | MARKS
         : c == Cause::WriteNodes    ? PAIR | WIDE_FILL | MARKS | OWN_TLAS | INST_REC
         : c == Cause::WriteTriVerts ? WIDE_FILL | MARKS
         : c == Cause::WriteXforms   ? OWN_TLAS | INST_REC
         : c == Cause::InstOption    ? (uint32_t)OWN_TLAS
         : 0u;
}
// ... and what hangs under a structure: deriving s anew makes these stale (the unified tree is re-derived with the own TLAS; new children lists need new boxes and leaf records)
constexpr uint32_t stale_with(Structure s) { return s == OWN_TLAS ? (uint32_t)UNI : s == WIDE_TOPO ? (uint32_t)WIDE_FILL : 0u; }

struct State {
    uint32_t valid = 0;
    // the packet walk's decision (host_launch.hpp packet_decide): 0 = probing (packets on, counters awaited), 1 = on, 2 = off
    int pkState = 0, pkBatchesSinceProbe = 0;
    void packet_reprobe() { pkState = 0; pkBatchesSinceProbe = 0; }
    void invalidate(Cause c) { valid &= ~stale_after(c); if (c == Cause::SceneReplaced) packet_reprobe(); }   // (another scene: the packet walk's decision is probed again)
    bool holds(Structure s) const { return (valid & s) == (uint32_t)s; }
    void mark(Structure s, bool on = true) { valid = on ? valid | s : valid & ~(uint32_t)s; }                   // a derivation's verdict: s is (or, on = false: turned out not to be) there
    void rederiving(Structure s) { valid &= ~stale_with(s); }                                                   // s is about to be derived anew
};
}   // namespace derived
