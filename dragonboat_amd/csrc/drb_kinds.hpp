// drb_kinds.hpp -- the step kernel's kinds, as one table, and the choice of
// the kinds a round launches (plan_step).  Everything that names a kind
// derives from the table: the StepKind enum, the launcher declarations and
// the launch table (drb_launch.hpp), the template arguments of each
// instantiation (drb_step_inst.hip) and the build's unit list
// (dragonboat_amd/build.py parses this file).  Host code only, on
// drb_layout.hpp alone (tests/native/step_plan.cpp compiles it with g++).
#pragma once
#include "drb_layout.hpp"

namespace drb {

// The values of R a kind is built for: X(R, K) per value.
#define DRB_FOR_ALL_R(X, K) \
  X(1, K) X(2, K) X(3, K) X(4, K) X(5, K) X(6, K) X(7, K) X(8, K)
// (the LOCAL kinds: the two shipped group sizes)
#define DRB_FOR_R3_R5(X, K) X(3, K) X(5, K)

// One row per kind: X(name, number, kernel, LEAD, EXT, SLOW, FWD, LOCAL,
// built for, stand-in).  `kernel` STEP is step_kernel<R, LEAD, EXT, SLOW,
// FWD, LOCAL> (drb_step.hpp), LEAN is lean_kernel<R, LEAD> (drb_lean.hpp: a
// listed round's heartbeat-only replicas).  EXT adds long Cmds, out-of-line
// values, EntryBatch / tan encoding, Quiesce, Snappy and sessions; SLOW is
// the raft launch (elections); FWD adds forwarded proposals
// (drb_config.forward_proposals) and the nonVoting / witness paths; LOCAL
// compiles the remote planes out (engines without placement,
// View.remote_mask 0).  A kind runs as its stand-in at every R outside
// "built for" (DRB_FOR_<set> above).  The numbers are part of the object
// and symbol names (step_r{R}_k{K}.o, step_launch_r{R}_k{K}).
#define DRB_STEP_KINDS(X)                                                  \
  X(LEAD, 0, STEP, 1, 0, 0, 0, 0, ALL_R, LEAD)                             \
  X(LEAD_EXT, 1, STEP, 1, 1, 0, 0, 0, ALL_R, LEAD_EXT)                     \
  X(FOLLOW, 2, STEP, 0, 0, 0, 0, 0, ALL_R, FOLLOW)                         \
  X(FOLLOW_EXT, 3, STEP, 0, 1, 0, 0, 0, ALL_R, FOLLOW_EXT)                 \
  X(SLOW, 4, STEP, 1, 1, 1, 1, 0, ALL_R, SLOW)                             \
  X(LEAD_FWD, 5, STEP, 1, 1, 0, 1, 0, ALL_R, LEAD_FWD)                     \
  X(FOLLOW_FWD, 6, STEP, 0, 1, 0, 1, 0, ALL_R, FOLLOW_FWD)                 \
  X(LEAD_LEAN, 7, LEAN, 1, 0, 0, 0, 0, ALL_R, LEAD_LEAN)                   \
  X(FOLLOW_LEAN, 8, LEAN, 0, 0, 0, 0, 0, ALL_R, FOLLOW_LEAN)               \
  X(LEAD_LOCAL, 9, STEP, 1, 0, 0, 0, 1, R3_R5, LEAD)                       \
  X(FOLLOW_LOCAL, 10, STEP, 0, 0, 0, 0, 1, R3_R5, FOLLOW)                  \
  X(LEAD_EXT_LOCAL, 11, STEP, 1, 1, 0, 0, 1, R3_R5, LEAD_EXT)              \
  X(FOLLOW_EXT_LOCAL, 12, STEP, 0, 1, 0, 0, 1, R3_R5, FOLLOW_EXT)

enum StepKind : int {
#define DRB_X(name, num, ...) SK_##name = num,
  DRB_STEP_KINDS(DRB_X)
#undef DRB_X
  NUM_STEP_KINDS
};

enum StepKernel { SKN_STEP, SKN_LEAN };

struct StepKindInfo {
  StepKernel kernel;  // (SKN_LEAN: lean_kernel<R, lead>, no other flag)
  bool lead, ext, slow, fwd, local;
  uint32_t built_for;  // bit R
  int stand_in;        // the kind that runs at the other R
};

constexpr StepKindInfo kStepKinds[NUM_STEP_KINDS] = {
#define DRB_X_BIT(R, K) | 1u << R
#define DRB_X(name, num, kernel, L, E, S, F, LOC, set, alt)              \
  {SKN_##kernel, L != 0, E != 0, S != 0, F != 0, LOC != 0,               \
   0u DRB_FOR_##set(DRB_X_BIT, num), SK_##alt},
    DRB_STEP_KINDS(DRB_X)
#undef DRB_X
#undef DRB_X_BIT
};

// the kind whose launcher runs `kind` with R replicas per group
constexpr int step_kind_at(int R, int kind) {
  return (kStepKinds[kind].built_for >> R) & 1u ? kind
                                                : kStepKinds[kind].stand_in;
}

// the largest round (workgroups of both launches) whose leader and
// follower launches run side by side (C2, 768 workgroups: 0.0882 against
// 0.0928 ms/round on one stream, profiles/r05_chunk)
constexpr uint64_t kSplitMaxBlocks = 2048;

// What one round launches (drb_engine.hip launch_step issues it).
struct StepPlan {
  int lead, follow;  // the two role launches' kinds
  bool split;  // the follower launch on the engine's second stream
  bool lean;   // the lean kinds first, the role launches then with LEAN_ALL
  bool slow;   // SK_SLOW follows
};

// nl / nf: the leader / follower launches' slot rows, gx: the round's group
// blocks; whole_round_on_engine_stream: not a chunk of drb_step_rounds and
// not on another stream; no_lean: drb_engine.no_lean.
inline StepPlan plan_step(const View &v, bool encode_saves, bool listed,
                          uint32_t nl, uint32_t nf, unsigned gx,
                          bool whole_round_on_engine_stream, bool no_lean) {
  // the EXT instantiation only where its paths can run (drb_step.hpp)
  const bool ext = v.C16 > 4 || v.kv_ool || encode_saves || v.quiesce ||
                   v.kv_ovf_cap || v.snappy || v.sessions;
  // forwarded proposals and member kinds: the EXT kernels with the Propose
  // and nonVoting / witness paths
  const bool fwd = v.fwd_props || v.nv_mask || v.wt_mask;
  // without placement (no remote planes) the LOCAL instantiations, which
  // compile the remote-plane paths out
  const bool local = !v.remote_mask;
  StepPlan p;
  p.lead = fwd ? SK_LEAD_FWD
           : ext ? (local ? SK_LEAD_EXT_LOCAL : SK_LEAD_EXT)
                 : (local ? SK_LEAD_LOCAL : SK_LEAD);
  p.follow = fwd ? SK_FOLLOW_FWD
             : ext ? (local ? SK_FOLLOW_EXT_LOCAL : SK_FOLLOW_EXT)
                   : (local ? SK_FOLLOW_LOCAL : SK_FOLLOW);
  // a small round (C2: 64k groups, 768 workgroups, one wave per SIMD) runs
  // its two launches side by side on the engine's two streams: they touch
  // disjoint state, and neither fills the chip alone
  p.split = nl && nf && whole_round_on_engine_stream && !v.elections &&
            (uint64_t)gx * (nl + nf) <= kSplitMaxBlocks;
  // listed rounds of a plain EXT engine: the light lanes' heartbeat rounds
  // through the lean kernel first (drb_lean.hpp), the full kernel then
  // over the heavy lanes and the ones the lean kernel escalated
  p.lean = listed && ext && !fwd && whole_round_on_engine_stream &&
           !v.elections && local && !v.save_tan && !v.save_batched &&
           !no_lean;
  // the replicas the two launches routed to the raft launch (F_SLOW)
  p.slow = v.elections != 0;
  return p;
}

}  // namespace drb
