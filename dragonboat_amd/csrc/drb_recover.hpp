// drb_recover.hpp -- drb_recover_tan on the device: replicas take their raft
// state, log window and state machine back from their tan logs.
//
//   node.replayLog (node.go:666-692)       the State and the entries of the
//     -> logdb ReadRaftState / tan         replica's logs (drb_tanread.hpp:
//        (internal/tan/db.go, open.go)     record reader, Update.Unmarshal,
//                                          overwrite and tail rules)
//   newRaft (internal/raft/raft.go:241-297), loadState (:446),
//   newEntryLog (logentry.go:86-95), newInMemory (inmemory.go:41-50),
//   Peer Launch (peer.go:64)               the restarted node: term, vote and
//                                          committed from the State, follower
//                                          (or the slot's nonVoting / witness
//                                          kind), no leader, ticks 0, remotes
//                                          reset, readIndex empty, a fresh
//                                          randomized timeout, inMemory empty
//                                          (markerIndex = last + 1, savedTo =
//                                          last), prevState the loaded State
//   the step loop's first apply            (snapshot index, committed] through
//                                          apply_entry (drb_step.hpp)
//
// One lane is one replica in both passes: every log is independent and is
// walked front to back (a record's place is known only from the chunk chain
// before it).  k_recover_check is pass 1 -- tr_validate, checksums included,
// nothing of the replica written but its plan; k_recover_place is pass 2 --
// tr_replay over the kept prefix with a placer that writes the window ring
// and applies, then the replica's state.  (A mapping that spreads a log's
// chunks over the lanes of a wave for the checksums was not built)
//
// The kernels are compiled in a translation unit of their own
// (drb_recover_inst.hip, DRB_RECOVER_KERNELS); the engine calls them through
// the launchers declared here.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/drb_engine.h"
#include "drb_layout.hpp"
#include "drb_tanread.hpp"

namespace drb {

// one log file as the kernels see it, replicas' files back to back in replica
// order q = slot * n_groups + (g - first_group), each replica's in log order
struct RecFile {
  uint64_t off, len;  // in RecParams.bytes (checked by the host)
  uint32_t log, pad;
};

struct RecParams {
  uint64_t first_group, n_groups;
  const uint8_t *bytes;
  const RecFile *files;
  const uint32_t *rep_first;  // [n_groups * R + 1]: replica q's files
  uint64_t base_index, base_term, seed;
  uint64_t qs_base;           // the engine's tick count
  TrPlan *plans;              // [n_groups * R], pass 1 -> pass 2
  drb_recover_status *st;     // [n_groups * R], (g - first_group) * R + slot
};

// what a call hands every replica: the entry the logs continue from, the
// seed of raft.rand, the engine's tick count
struct RecBase {
  uint64_t base_index, base_term, seed, qs_base;
};

// a workgroup is one wave: replicas' logs differ in length
constexpr uint32_t REC_BLOCK = 64;

void recover_launch_check(const View &v, const RecParams &p, unsigned blocks,
                          hipStream_t s);
void recover_launch_place(const View &v, const RecParams &p, unsigned blocks,
                          hipStream_t s);

// a replica's files: files[k] is a TanFile over the uploaded bytes
struct RecFiles {
  const uint8_t *bytes;
  const RecFile *f;
  __host__ __device__ TanFile<TanFlatIn> operator[](uint32_t k) const {
    return TanFile<TanFlatIn>{TanFlatIn{bytes}, f[k].off, f[k].len};
  }
};

}  // namespace drb

#ifdef DRB_RECOVER_KERNELS
#include "drb_step.hpp"  // apply_entry

namespace drb {

// lane -> replica of the call
__device__ __forceinline__ bool rec_lane(const View &v, const RecParams &p,
                                         uint64_t *q, uint32_t *slot,
                                         uint64_t *g) {
  *q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (*q >= p.n_groups * v.R) return false;
  *slot = (uint32_t)(*q / p.n_groups);
  *g = p.first_group + (*q - (uint64_t)*slot * p.n_groups);
  return true;
}

__device__ __forceinline__ TrLimits rec_limits(const View &v,
                                               const RecParams &p,
                                               uint32_t slot, uint64_t g) {
  TrLimits lim;
  lim.shard_id = v.first_shard_id + gid(v, slot, g);
  lim.replica_id = slot + 1;
  lim.base_index = p.base_index;
  lim.cmd_cap = v.C16 * 16;
  lim.W = v.W;
  lim.snappy = v.snappy;
  lim.sessions = v.sessions;
  return lim;
}

// ------------------------------------------------------------ pass 1
__global__ __launch_bounds__(REC_BLOCK) void k_recover_check(View v,
                                                             RecParams p) {
  uint64_t q, g;
  uint32_t slot;
  if (!rec_lane(v, p, &q, &slot, &g)) return;
  const uint32_t f0 = p.rep_first[q], nf = p.rep_first[q + 1] - f0;
  const RecFiles files{p.bytes, p.files + f0};
  TrPlan pl;
  if (gid(v, slot, g) < v.total_groups)
    pl = tr_validate(files, nf, rec_limits(v, p, slot, g));
  p.plans[q] = pl;
  drb_recover_status st;
  st.status = pl.status;
  st.log = pl.files ? p.files[f0 + pl.files - 1].log : 0;
  st.offset = pl.offset;
  st.records = pl.records;
  st.entries = pl.entries;
  st.term = pl.term;
  st.vote = pl.vote;
  st.commit = pl.commit;
  st.last_index = pl.last_index;
  st.applied = 0;
  p.st[(g - p.first_group) * v.R + slot] = st;
  if (pl.status >= TRS_CORRUPT) {  // refused: the CPU path restarts it
    v.u32[u32_ix(v, W_FLAGS, slot, g)] |= DRB_F_FALLBACK;
    v.u32[u32_ix(v, W_FB_REASON, slot, g)] = DRB_FB_RECOVERY;
  }
}

// ------------------------------------------------------------ pass 2
// tr_replay's placer over the resident window of replica (slot, g): a Cmd
// goes out as 16 B chunks as its bytes come in, the rest of the entry's Cmd
// chunks are zeroed (as drb_import_log leaves them), then its three meta
// chunks; apply is the step kernel's apply_entry (the EXT instantiation:
// long Cmds, out-of-line values, Snappy).
struct RingPlacer {
  const View &v;
  Lane L;
  Rep<1> r;
  uint64_t base;
  uint64_t term_final;  // the State's term
  uint64_t term_start;  // every placed entry in [term_start, last] has it
  int stop = 0;         // apply_entry's refusal

  __device__ RingPlacer(const View &view, uint32_t slot, uint64_t g,
                        uint64_t base_index, uint64_t base_term, uint64_t term)
      : v(view), base(base_index), term_final(term) {
    L = Lane();
    L.v = &view;
    L.slot = slot;
    L.g = g;
    L.tid = threadIdx.x;
    r = Rep<1>();
    r.sm_index = base_index;
    r.sm_term = base_term;
    term_start = base_term == term ? base_index : base_index + 1;
  }

  __device__ __forceinline__ void chunk(uint64_t index, uint32_t c, uint64_t lo,
                                        uint64_t hi) {
    if (c < v.C16)  // (pass 1 bounded cmd_len by the window's Cmd chunks)
      v.ring[ring_ix(v, L.slot, index, ENT_META + c, L.g)] =
          make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi,
                     (uint32_t)(hi >> 32));
  }

  template <class C>
  __device__ void cmd(C &c, const TrEntry &e) {
    if (e.index <= base || e.cmd_len > v.C16 * 16) {
      c.skip(e.cmd_len);
      return;
    }
    uint64_t lo = 0, hi = 0;
    for (uint32_t i = 0; i < e.cmd_len; ++i) {
      const uint64_t b = c.byte();
      const uint32_t k = i & 15;
      if (k < 8)
        lo |= b << (8 * k);
      else
        hi |= b << (8 * (k - 8));
      if (k == 15 || i + 1 == e.cmd_len) {
        chunk(e.index, i >> 4, lo, hi);
        lo = hi = 0;
      }
    }
  }

  __device__ void place(const TrEntry &e) {
    for (uint32_t c = (e.cmd_len + 15) / 16; c < v.C16; ++c)
      chunk(e.index, c, 0, 0);
    v.ring[ring_ix(v, L.slot, e.index, 0, L.g)] = mk4(e.term, e.key);
    v.ring[ring_ix(v, L.slot, e.index, 1, L.g)] =
        mk4(e.client_id, e.series_id);
    uint4 m2 = mk4(e.responded_to, 0);
    m2.z = e.type;
    m2.w = e.cmd_len;
    v.ring[ring_ix(v, L.slot, e.index, 2, L.g)] = m2;
    // the log now ends at e.index
    if (e.term != term_final)
      term_start = e.index + 1;
    else if (term_start > e.index)
      term_start = e.index;
  }

  __device__ bool apply(uint64_t index) {
    const int rc = apply_entry<1, true>(L, r, index);
    if (rc < 0) stop = rc;
    return rc >= 0;
  }
};

// The end of pass 2 for replica (slot, g), behind the replay (`ok`: it ran
// through; `applied`: its apply cursor): the KV count, then the restarted
// node's state -- or, when the apply stopped, the fallback mark.  tan_state
// is what the replica's tan_st becomes (save_tan).  Shared by the regular
// and the multiplexed recovery (drb_recover_mux.hpp).
__device__ inline void rec_place_finish(const View &v, const RecBase &p,
                                        uint32_t slot, uint64_t g,
                                        const TrPlan &pl, RingPlacer &pc,
                                        bool ok, uint64_t applied,
                                        drb_recover_status &st,
                                        uint4 tan_state) {
  st.applied = applied;
  // KVTest.Count: the updates applied, and what the replica's record had
  // counted since the field was last written (word 15's delta, which the
  // record loses below or keeps zeroed here)
  {
    uint4 c3 = v.pk[pk_ix(v, 3, slot, g)];
    v.u64[u64_ix(v, F_KV_COUNT, slot, g)] += pc.r.kv_added + (c3.w >> 16);
    c3.w &= 0xffffu;
    v.pk[pk_ix(v, 3, slot, g)] = c3;
  }
  if (!ok) {  // the KV filled (or refused a payload) part way
    st.status = TRS_APPLY_STOPPED;
    v.u32[u32_ix(v, W_FLAGS, slot, g)] |= DRB_F_FALLBACK;
    v.u32[u32_ix(v, W_FB_REASON, slot, g)] = DRB_FB_RECOVERY;
    return;
  }
  const uint64_t last = pl.last_index, commit = pl.commit;
  // the entry the log continues from stays readable (a Replicate's
  // prevLogTerm) while the window has room for it
  // What the ring still holds starts W below the highest index ever placed,
  // not below the last one: a tail that an overwrite cut off again took the
  // slots of index - W on its way (TrReplay).  The last entry itself is
  // always the latest occupant of its slot.
  const uint64_t high = pl.high_index > last ? pl.high_index : last;
  uint64_t ring_lo = high + 1 > v.W ? high + 1 - v.W : 1;
  if (ring_lo > last) ring_lo = last ? last : 1;
  if (ring_lo <= p.base_index) {
    ring_lo = p.base_index ? p.base_index : 1;
    if (p.base_index) {
      for (uint32_t c = 0; c < v.C16; ++c) pc.chunk(p.base_index, c, 0, 0);
      v.ring[ring_ix(v, slot, p.base_index, 0, g)] = mk4(p.base_term, 0);
      v.ring[ring_ix(v, slot, p.base_index, 1, g)] = mk4(0, 0);
      v.ring[ring_ix(v, slot, p.base_index, 2, g)] = mk4(0, 0);
    }
  }
  uint64_t term_start = pc.term_start < ring_lo ? ring_lo : pc.term_start;
  if (term_start > last + 1) term_start = last + 1;
  // raft.rand seeded as drb_init_steady seeds it, then one draw for the
  // randomized election timeout (reset -> setRandomizedElectionTimeout,
  // raft.go:658-661; el_rand_timeout)
  uint64_t rng = mix64(p.seed ^ (0xE2ull << 56) ^ (gid(v, slot, g) * v.R + slot));
  rng += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  uint64_t vals[NUM_U64], over[NUM_U64];
  for (int k = 0; k < NUM_U64; ++k) vals[k] = over[k] = 0;
  vals[F_TERM] = pl.term;
  vals[F_VOTE] = pl.vote;
  vals[F_RAND_TIMEOUT] = v.election_rtt + z % v.election_rtt;
  vals[F_COMMITTED] = commit;
  vals[F_PROCESSED] = commit;
  vals[F_APPLIED] = commit;
  vals[F_LAST_INDEX] = last;
  vals[F_MARKER_INDEX] = last + 1;
  vals[F_SAVED_TO] = last;
  vals[F_APPLIED_INDEX] = commit;
  vals[F_CONFIRMED_INDEX] = commit;
  vals[F_PUSHED_INDEX] = commit;
  vals[F_PREV_TERM] = pl.term;
  vals[F_PREV_VOTE] = pl.vote;
  vals[F_PREV_COMMIT] = commit;
  vals[F_SM_INDEX] = commit;
  vals[F_SM_TERM] = pc.r.sm_term;
  vals[F_RING_LO] = ring_lo;
  vals[F_RING_GUARD] = ~0ull;
  vals[F_TERM_START] = term_start;
  uint32_t w[16];
  pk_encode(w, vals, over);
  for (int k = 0; k < NUM_U64; ++k) {
    const bool counter = k == F_TICK_COUNT || k == F_KV_COUNT ||
                         (k >= F_QS_TICK && k <= F_QS_EXIT) || k == F_RNG ||
                         k == F_QS_BASE || k == F_SAVE_BASE;
    if (!counter) v.u64[u64_ix(v, k, slot, g)] = over[k] ? over[k] : vals[k];
  }
  for (int ch = 0; ch < 4; ++ch)
    v.pk[pk_ix(v, ch, slot, g)] =
        make_uint4(w[4 * ch], w[4 * ch + 1], w[4 * ch + 2], w[4 * ch + 3]);
  v.u64[u64_ix(v, F_TICK_COUNT, slot, g)] = 0;
  for (int f = F_QS_TICK; f <= F_QS_EXIT; ++f) v.u64[u64_ix(v, f, slot, g)] = 0;
  v.u64[u64_ix(v, F_QS_BASE, slot, g)] = p.qs_base;
  v.u64[u64_ix(v, F_SAVE_BASE, slot, g)] = 0;
  v.u64[u64_ix(v, F_RNG, slot, g)] = rng;
  v.u32[u32_ix(v, W_ROLE, slot, g)] = (v.nv_mask >> slot) & 1u ? DRB_NONVOTING
                                      : (v.wt_mask >> slot) & 1u ? DRB_WITNESS
                                                                 : DRB_FOLLOWER;
  v.u32[u32_ix(v, W_FLAGS, slot, g)] = DRB_F_HOSTED;
  v.u32[u32_ix(v, W_FB_REASON, slot, g)] = 0;
  v.u32[u32_ix(v, W_RI_COUNT, slot, g)] = 0;
  v.u32[u32_ix(v, W_VOTES, slot, g)] = 0;
  for (uint32_t peer = 0; peer < v.R; ++peer) {  // resetRemotes
    v.rem_match[rem_ix(v, slot, peer, g)] = 0;
    v.rem_next[rem_ix(v, slot, peer, g)] = last + 1;
    v.rem_state[rem_ix(v, slot, peer, g)] = DRB_REMOTE_RETRY;
    v.rem_active[rem_ix(v, slot, peer, g)] = 0;
  }
  if (v.save_tan) v.tan_st[ix(v, slot, g)] = tan_state;
}

__global__ __launch_bounds__(REC_BLOCK) void k_recover_place(View v,
                                                             RecParams p) {
  uint64_t q, g;
  uint32_t slot;
  if (!rec_lane(v, p, &q, &slot, &g)) return;
  const TrPlan pl = p.plans[q];
  if (pl.status != TRS_OK && pl.status != TRS_TAIL_CUT) return;
  const uint32_t f0 = p.rep_first[q];
  const RecFiles files{p.bytes, p.files + f0};
  drb_recover_status &st = p.st[(g - p.first_group) * v.R + slot];
  RingPlacer pc(v, slot, g, p.base_index, p.base_term, pl.term);
  uint64_t applied = p.base_index;
  const bool ok =
      tr_replay(files, pl, rec_limits(v, p, slot, g), pc, &applied);
  // the tan writer goes on behind the last kept record
  rec_place_finish(v, RecBase{p.base_index, p.base_term, p.seed, p.qs_base},
                   slot, g, pl, pc, ok, applied, st,
                   make_uint4((uint32_t)pl.offset, (uint32_t)(pl.offset >> 32),
                              st.log, pl.state_stored ? 1u /*TST_STATE*/ : 0u));
}

}  // namespace drb
#endif  // DRB_RECOVER_KERNELS
