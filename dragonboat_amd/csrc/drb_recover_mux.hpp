// drb_recover_mux.hpp -- drb_recover_tan_mux on the device: replicas of a
// tan_multiplexed engine take their state back from the 16 shared logs of
// their slot (drb_tanmux.hpp has the rules and the bodies).
//
// A shared log is few and long (C3: 48 logs of about 80 MB), so the walk is
// spread over its 32 KiB blocks and the records are then handed out:
//
//   k_mux_index     pass A, one lane per block of every file: the block's
//                   two-state summary, every checksum verified
//   k_mux_compose   one lane per log: its files' summaries in order -> each
//                   block's entry state and kept record count, the log's
//                   chunk-level status and writer position
//   (exclusive scan of the counts: the record numbers, in log order)
//   k_mux_records   pass B, one lane per block: a descriptor per kept record
//                   and its owner q = slot * G + g as the sort key
//   (stable radix sort of (q, record number) on q's bits: every replica's
//   records in log order, no atomics on the way)
//   k_mux_check     one lane per replica: its span of the sorted list (two
//                   binary searches), tm_validate; the statuses
//   k_mux_place     one lane per replica: tm_replay with RingPlacer, then
//                   rec_place_finish -- the tail k_recover_place ends with;
//                   the logs' writers
//
// The kernels are compiled in drb_recover_inst.hip (DRB_RECOVER_KERNELS);
// the engine calls them through the launchers declared here.
#pragma once
#include "drb_recover.hpp"
#include "drb_tanmux.hpp"

namespace drb {

struct MuxParams {
  const uint8_t *bytes;
  const TmFile *files;        // [n_files] by log L = slot * 16 + key, each
                              // log's in log order
  const uint32_t *log_first;  // [R * 16 + 1]: log L's files
  const uint32_t *file_log;   // [n_files]: L
  const uint32_t *blk_file;   // [n_blocks]: the block's file
  uint32_t n_files, n_blocks, n_logs, n_recs;
  TmBlock *sums;              // [n_blocks], pass A
  uint8_t *entry;             // [n_blocks], the composition
  uint32_t *cnt, *first;      // [n_blocks]: kept records, their first number
  TmLogOut *logs;             // [n_logs]
  // the first record in log order whose owner refuses the log:
  // (record number << 8) | status, ~0 none
  unsigned long long *log_bad;  // [n_logs]
  TmRec *recs;                  // [n_recs]
  uint32_t *keys, *vals;        // [n_recs] (q, record number), pass B
  const uint32_t *skeys, *svals;  // sorted
  uint2 *rep;                   // [G * R] {first, count} in the sorted list
  RecBase base;
  TrPlan *plans;               // [G * R]
  drb_recover_status *st;      // [G * R], g * R + slot
  drb_recover_log_status *lst; // [n_logs]
};

void recover_mux_index(const View &v, const MuxParams &p, hipStream_t s);
// the scan's / the sort's temporary bytes (n items, keys below `bound`)
size_t recover_mux_scan_temp(uint32_t n);
size_t recover_mux_sort_temp(uint32_t n, uint64_t bound);
hipError_t recover_mux_scan(const MuxParams &p, void *tmp, size_t tmp_bytes,
                            hipStream_t s);
void recover_mux_records(const View &v, const MuxParams &p, hipStream_t s);
// keys / vals -> keys_out / vals_out
hipError_t recover_mux_sort(const MuxParams &p, uint32_t *keys_out,
                            uint32_t *vals_out, uint64_t bound, void *tmp,
                            size_t tmp_bytes, hipStream_t s);
void recover_mux_check(const View &v, const MuxParams &p, hipStream_t s);
void recover_mux_place(const View &v, const MuxParams &p, hipStream_t s);

}  // namespace drb

#ifdef DRB_RECOVER_KERNELS
namespace drb {

__device__ __forceinline__ TanFile<TanFlatIn> mux_file(const MuxParams &p,
                                                       uint32_t fi) {
  return TanFile<TanFlatIn>{TanFlatIn{p.bytes}, p.files[fi].off,
                            p.files[fi].len};
}

// Pass A.  A lane streams its own 32 KiB block front to back (the chunk
// chain inside a block is sequential), the payload through 8-byte get64
// loads in tr_xxh64.  The lanes of a wave stand 32 KiB apart, so their loads
// are NOT coalesced: each lane's load opens a cache line of its own that its
// next seven loads then hit.  What a wave's lanes share is the file table
// alone.  One wave per workgroup: blocks differ in how many chunks they hold.
__global__ __launch_bounds__(REC_BLOCK) void k_mux_index(MuxParams p) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.n_blocks) return;
  const uint32_t fi = p.blk_file[b];
  p.sums[b] = tm_summarize(mux_file(p, fi), b - p.files[fi].blk0);
}

__global__ __launch_bounds__(REC_BLOCK) void k_mux_compose(MuxParams p) {
  const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
  if (L >= p.n_logs) return;
  const uint32_t f0 = p.log_first[L];
  p.logs[L] = tm_compose_log(p.files + f0, p.log_first[L + 1] - f0, p.sums,
                             p.entry, p.cnt, nullptr);
  p.log_bad[L] = ~0ull;
}

// pass B's emit: record i of the block
struct MuxEmit {
  const View &v;
  const MuxParams &p;
  TanFile<TanFlatIn> f;
  uint32_t fi, L, first;
  __device__ void operator()(uint32_t i, uint64_t hdr) {
    const uint32_t no = first + i;
    uint64_t rlen = 0, end, shard, replica, g = 0;
    uint32_t st = tm_record(f, hdr, &rlen, &end, &shard, &replica);
    if (st == TRS_OK)
      st = tm_owner_status(shard, replica, v.first_shard_id, v.G,
                           L / TM_KEYS, L % TM_KEYS, &g);
    if (st != TRS_OK)  // (rare: the one atomic of the call)
      atomicMin(&p.log_bad[L], ((unsigned long long)no << 8) | st);
    p.recs[no] = TmRec{hdr, fi, (uint32_t)rlen};
    p.keys[no] = st == TRS_OK ? (uint32_t)((L / TM_KEYS) * v.G + g)
                              : (uint32_t)(v.G * v.R);
    p.vals[no] = no;
  }
};

// Pass B.  As pass A without the hashing; a record's chunks are followed
// into the blocks behind its own for its payload length.
__global__ __launch_bounds__(REC_BLOCK) void k_mux_records(View v,
                                                           MuxParams p) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.n_blocks) return;
  const uint32_t n = p.cnt[b];
  if (n == 0) return;
  const uint32_t fi = p.blk_file[b];
  MuxEmit emit{v, p, mux_file(p, fi), fi, p.file_log[fi], p.first[b]};
  tm_block_records(emit.f, b - p.files[fi].blk0, p.entry[b], n, emit);
}

// the first position of the sorted keys that is not below q
__device__ __forceinline__ uint32_t mux_lower(const uint32_t *keys, uint32_t n,
                                              uint32_t q) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < q)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// a log's status: its chunks', else what the first foreign record says
__device__ __forceinline__ uint32_t mux_log_status(const MuxParams &p,
                                                   uint32_t L) {
  const uint32_t st = p.logs[L].status;
  const unsigned long long bad = p.log_bad[L];
  if (st >= TRS_CORRUPT || st == TRS_EMPTY || bad == ~0ull) return st;
  return (uint32_t)(bad & 0xffu);
}

__device__ __forceinline__ TrLimits mux_limits(const View &v,
                                               const MuxParams &p,
                                               uint32_t slot, uint64_t g) {
  TrLimits lim;
  lim.shard_id = v.first_shard_id + gid(v, slot, g);
  lim.replica_id = slot + 1;
  lim.base_index = p.base.base_index;
  lim.cmd_cap = v.C16 * 16;
  lim.W = v.W;
  lim.snappy = v.snappy;
  lim.sessions = v.sessions;
  return lim;
}

// Pass 1: lane i is replica q = i (slot = q / G, g = q % G) and, below
// n_logs, also reports log i.  Nothing of a replica is written but its plan
// (and the fallback mark of a refused one).
__global__ __launch_bounds__(REC_BLOCK) void k_mux_check(View v, MuxParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p.n_logs) {
    const TmLogOut lo = p.logs[i];
    drb_recover_log_status ls;
    ls.status = mux_log_status(p, (uint32_t)i);
    ls.log = lo.log;
    ls.offset = lo.offset;
    ls.records = lo.records;
    p.lst[i] = ls;
  }
  if (i >= v.G * v.R) return;
  const uint32_t slot = (uint32_t)(i / v.G);
  const uint64_t g = i - (uint64_t)slot * v.G;
  // (tanm_key, drb_tan.hpp: place_world 1, ShardID = first_shard_id + g)
  const uint32_t L =
      slot * TM_KEYS + (uint32_t)((v.first_shard_id + g) % TM_KEYS);
  const TmLogOut lo = p.logs[L];
  const uint32_t lstat = mux_log_status(p, L);
  TrPlan pl;
  uint2 rep = make_uint2(0, 0);
  if (lstat == TRS_OK || lstat == TRS_TAIL_CUT) {
    rep.x = mux_lower(p.skeys, p.n_recs, (uint32_t)i);
    rep.y = mux_lower(p.skeys, p.n_recs, (uint32_t)i + 1) - rep.x;
    const TmRecList list{p.bytes, p.files, p.recs, p.svals + rep.x};
    pl = tm_validate(list, rep.y, mux_limits(v, p, slot, g));
  } else {
    pl.status = lstat;
  }
  p.rep[i] = rep;
  p.plans[i] = pl;
  drb_recover_status st;
  st.status = pl.status;
  st.log = lo.log;  // the log's writer
  st.offset = lo.offset;
  st.records = pl.records;
  st.entries = pl.entries;
  st.term = pl.term;
  st.vote = pl.vote;
  st.commit = pl.commit;
  st.last_index = pl.last_index;
  st.applied = 0;
  p.st[g * v.R + slot] = st;
  if (pl.status >= TRS_CORRUPT) {  // refused: the CPU path restarts it
    v.u32[u32_ix(v, W_FLAGS, slot, g)] |= DRB_F_FALLBACK;
    v.u32[u32_ix(v, W_FB_REASON, slot, g)] = DRB_FB_RECOVERY;
  }
}

// Pass 2, and the writers of the logs that stand
__global__ __launch_bounds__(REC_BLOCK) void k_mux_place(View v, MuxParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p.n_logs) {
    const uint32_t lstat = mux_log_status(p, (uint32_t)i);
    if (lstat == TRS_OK || lstat == TRS_TAIL_CUT) {
      const TmLogOut lo = p.logs[i];
      v.tanm_cur[i] = make_uint4((uint32_t)lo.offset,
                                 (uint32_t)(lo.offset >> 32), lo.log, 0);
    }
  }
  if (i >= v.G * v.R) return;
  const TrPlan pl = p.plans[i];
  if (pl.status != TRS_OK) return;
  const uint32_t slot = (uint32_t)(i / v.G);
  const uint64_t g = i - (uint64_t)slot * v.G;
  const uint2 rep = p.rep[i];
  const TmRecList list{p.bytes, p.files, p.recs, p.svals + rep.x};
  drb_recover_status &st = p.st[g * v.R + slot];
  RingPlacer pc(v, slot, g, p.base.base_index, p.base.base_term, pl.term);
  uint64_t applied = p.base.base_index;
  const bool ok =
      tm_replay(list, rep.y, pl, mux_limits(v, p, slot, g), pc, &applied);
  // the replica's stored-State flag; its writer is its log's (tanm_cur)
  uint4 ts = v.tan_st[ix(v, slot, g)];
  ts.w = pl.state_stored ? 1u /*TST_STATE*/ : 0u;
  rec_place_finish(v, p.base, slot, g, pl, pc, ok, applied, st, ts);
}

}  // namespace drb
#endif  // DRB_RECOVER_KERNELS
