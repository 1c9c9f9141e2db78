// walk_plan.hpp — which traversal walk the launches of a batch (or of one idkptTraceRays call) get: the decision as pure code.  Nothing from HIP and no dev_ctx in here: g++ compiles this header
// on its own (tests/test_walk_plan.py).  The host side — host_launch.hpp trace_plan — fills WalkInputs from the context and derives what the candidates need; launch_trace2 launches what the plan says.
#pragma once
#include <algorithm>
#include <stddef.h>
#include <stdint.h>
namespace walk {
// What ships, walk by walk (P: primary / bounce launch, C: counting build, V: scene versions; "+ flagged": the rays the walk does not vouch for are traced again, exactly, right behind it).  Everything else the
// kernel templates can express is unreachable from launch_trace2; developer builds (-DIDKPT_DEVELOPER, option "trace_variant") add instrumented and probe instantiations.
//   walk     kernel instantiation(s)                                             conditions                                                                                by default
//   Generic  k_trace_primary / k_trace_queue; k_trace_query                      debug view, force_generic; queries with query_scheduler = 0 (never through launch_trace2)  off
//   Plain    k_trace2<P, C, 32, 1, false, 24, 0, 0 | 16, V>                      one BLAS instance (MODE 0); leaf phase plain or pooled per bounce (leaf_pool)              counters, versions, queries
//   Fast     k_trace2<P, false, 32, 1, false, 24, 0, 0 | 16, false, false, true> ... on the regrouped pairs: frames, one scene version, no counters (pair_nodes)           on
//   Loop     k_trace2<P, C, 16, 1, false, 24, 1, 0, V>                           several instances: the reference's instance loop (MODE 1)                                  2-7 instances, counters, versions
//   Tlas     k_trace2<P, C, 16, 1, false, 24, 2, 0, V>                           UseTlas: the host's TLAS (MODE 2)                                                          with UseTlas
//   Wide     k_trace_wide<P, C'> + flagged                                       one BLAS, option wide = 1 (C': wide_count)                                                 off
//   OwnTlas  k_trace_inst<P> + flagged                                           inst_tlas (8) .. 4096 instances whose boxes overlap little (inst_tlas_overlap)             on
//   Unified  k_trace_inst<P, false, 16 | 32, 1> + flagged                        2 .. 1024 instances in one space, each BLAS used once (inst_unify; refill: uni_refill)     on; inst_tlas = 0 does NOT turn it off, only inst_unify = 0 does
//   General  k_trace_inst<P, false, 16, 2> + flagged                             inst_general .. 1024 instances that are not one space                                      off
//   Sieve    k_trace_inst<P, true>                                               inst_sieve (8) .. 1024 instances that keep the loop (inst_sieve_overlap)                   on; closest-hit queries: wherever a frame would take OwnTlas / Unified / General / Sieve
// On top of the batch's walk, per launch:
//   any-hit queries  k_trace2<true, false, 32, 1, false, 24, M, 0, false, true>, M = 0 / 1 / 2 by scene shape (Plain / Loop / Tlas)
//   packetPrimary    k_trace_packet<true[, true]> + k_packet_mirror + flagged: the primary launch of bounce 0 on one BLAS or on the unified tree (option packet: 1 = by measurement, the default)
//   occlusion        k_trace2<P, false, 32, 1, false, 24, 0, 0 | 16, false, false, false | true, true> instead of Plain / Fast: the deferred last bounce where only hit-or-miss of it is read (option last_occlusion, host_schedule.hpp flush_batch)
//   split            k_trace2s<P> instead of Plain / Fast: small launches of sparse views (want_split);   fused: k_trace_fused<32> instead of both launches of a RayDepth-2 batch (default off)
//   flagged          one BLAS: k_trace2<P, false>; several instances: k_trace_inst<P, true> while a lane's mask fits its LDS rows, else k_trace2<P, false, 16, 1, false, 24, 1, 0, false>
enum class Walk { Generic, Plain, Fast, Loop, Tlas, Wide, OwnTlas, Unified, General, Sieve };
struct WalkInputs {
    int instanceCount; bool useTlas, debugView; int verSlots; bool counters, sceneNested;                              // the scene and the settings
    int wide, pairNodes, packet, instTlas, instSieve, instUnify, traceVariant; bool forceGeneric, queryScheduler;      // DevOptions
    bool multiVer, pixelMajor, query, anyHit;                                                                          // this batch / this idkptTraceRays call
    bool itlasValid, itlasBuilt, isieveWorth, uniValid; int uniMode, maskWords, maskRows;                              // what the derivations on the device reported
};
struct TracePlan { Walk walk; bool packetPrimary, fused, multiVer, counting, anyHit, splitOk, retraceSieved; size_t ldsBytes; int wavesPerCU; uint32_t grid; };   // what launch_trace2 is handed: the walk of the closest-hit launches and what goes on top of it
inline bool stock_variant(const WalkInputs& in) { return in.traceVariant == 0 || in.traceVariant == 100; }
// the persistent while-while traversal (one BLAS, instance list or TLAS); only the debug traversal-cost view and force_generic use the general kernels
inline bool fast_path(const WalkInputs& in) { return in.instanceCount >= 1 && !in.debugView && !in.forceGeneric; }
// What every optional walk asks for: closest hit without UseTlas, no debug view, one scene version, the reference's counters not asked for, stock kernels.  wideRules: the wide-node walk does not look at the debug view (it is only asked behind fast_path) and accepts the instrumented variant 213.
inline bool optional_walks_allowed(const WalkInputs& in, bool wideRules = false) { return !in.useTlas && (wideRules || !in.debugView) && in.verSlots == 1 && !in.counters && (stock_variant(in) || (wideRules && in.traceVariant == 213)); }
inline bool wide_wanted(const WalkInputs& in) { return in.wide != 0 && in.instanceCount == 1 && optional_walks_allowed(in, true); }
inline bool pair_nodes_wanted(const WalkInputs& in) { return in.pairNodes != 0 && in.instanceCount == 1 && !in.forceGeneric && optional_walks_allowed(in); }
// one BLAS, or the unified tree of a same-space scene; boxes that nest (the packet walk's lenient inner-box test needs it)
inline bool packet_possible(const WalkInputs& in) { return in.packet != 0 && (in.instanceCount == 1 || (in.uniValid && in.uniMode == 1 && in.itlasValid && in.itlasBuilt)) && in.sceneNested && !in.forceGeneric && optional_walks_allowed(in); }
// the own TLAS — or, sieve: the exact loop with the instance sieve.  (A lane's mask has 32 LDS rows; k_tlas_build is one workgroup: beyond a few thousand instances its cost per transform update is not the loop's business)
inline bool inst_tlas_wanted(const WalkInputs& in, bool sieve = false) { const int from = sieve ? in.instSieve : in.instTlas; return in.instanceCount <= (sieve ? 1024 : 4096) && from > 0 && in.instanceCount >= std::max(2, from) && optional_walks_allowed(in); }
// the unified tree: from two instances on, BLAS boxes that nest (inst_unify_prepare checks the rest: one space, every BLAS used once)
inline bool inst_unify_wanted(const WalkInputs& in) { return in.instUnify > 0 && in.instanceCount >= 2 && in.instanceCount <= 1024 && in.sceneNested && optional_walks_allowed(in); }
// what inst_unify_prepare derives for n instances: 1 = one space, the unified tree (TREE 1); otherwise — different transforms, or a BLAS instanced several times — 2 = the general array (TREE 2), or nothing
inline int unify_mode(bool sameSpace, int n, int instGeneral) { return sameSpace ? 1 : (instGeneral > 0 && n >= instGeneral ? 2 : 0); }
// several instances without UseTlas, after inst_tlas_derive: through a tree (the unified one wins where it exists), by the exact loop with the sieve, or by k_trace2 MODE 1
inline Walk inst_walk(const WalkInputs& in)
{
    if (in.itlasBuilt && (in.uniValid ? inst_unify_wanted(in) : inst_tlas_wanted(in))) return !in.uniValid ? Walk::OwnTlas : in.uniMode == 2 ? Walk::General : Walk::Unified;
    return inst_tlas_wanted(in, true) && (in.isieveWorth || in.itlasBuilt) ? Walk::Sieve : Walk::Loop;
}
inline Walk shape_walk(const WalkInputs& in) { return in.useTlas ? Walk::Tlas : in.instanceCount > 1 ? Walk::Loop : Walk::Plain; }
inline Walk choose_walk(const WalkInputs& in)
{
    if (in.query && (!in.queryScheduler || in.debugView)) return Walk::Generic;
    if (in.query) return !in.anyHit && in.instanceCount > 1 && !in.useTlas && inst_walk(in) != Walk::Loop ? Walk::Sieve : shape_walk(in);   // closest hits take the sieve where a frame would take it or a tree; no Wide, no Fast
    if (!fast_path(in)) return Walk::Generic;
    if (wide_wanted(in)) return Walk::Wide;
    if (inst_walk(in) != Walk::Loop) return inst_walk(in);
    return !in.multiVer && pair_nodes_wanted(in) ? Walk::Fast : shape_walk(in);
}
// The packet walk on a batch's primary launch: forbidden, forced (packet = 2), or — pixel-major lists only — up to the kernel's own counters (packet_decide's state machine)
enum class PacketVote { No, Yes, Measure }; inline PacketVote packet_vote(const WalkInputs& in) { return !packet_possible(in) ? PacketVote::No : in.packet >= 2 ? PacketVote::Yes : in.pixelMajor ? PacketVote::Measure : PacketVote::No; }
inline bool packet_primary(const WalkInputs& in, Walk w, bool packetBatch /* Frame::packet: the vote went its way and the batch is not fused */) { return packetBatch && (in.instanceCount == 1 || w == Walk::Unified); }
inline bool split_allowed(const WalkInputs& in, Walk w) { return (w == Walk::Plain || w == Walk::Fast) && !in.multiVer && !in.counters && in.sceneNested && stock_variant(in); }
}   // namespace walk
