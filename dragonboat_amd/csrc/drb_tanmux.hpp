// drb_tanmux.hpp -- the read path of the multiplexed tan LogDB: a shared log
// (16 per replica slot, keyed by ShardID % 16; internal/tan/db.go, a shared
// db rebuilds one log for all its nodes, open.go:200-268, db_keeper.go:84-123)
// is indexed block by block, its records are handed to the replicas that own
// them, and each replica replays its own subsequence by the per-record bodies
// of drb_tanread.hpp.  One body for the host and the device, as that header.
//
//   block index     A tan file is a sequence of 32 KiB blocks; a chunk never
//                   leaves its block and the writer pads a block's end.  So
//                   the chunks of a block follow from its bytes and the file
//                   size alone.  What the reader carries across blocks is one
//                   bit: between records (it wants a FULL / FIRST chunk and
//                   skips others) or inside one (any chunk continues it, a
//                   FULL / LAST one ends it).  tm_summarize walks a block once
//                   -- through tr_next_chunk on the block as a file of its
//                   own, so a chunk is accepted or refused by the reader's own
//                   rules, every checksum verified as the sequential reader
//                   verifies the chunks it skips -- and records for both entry
//                   states the exit state, the records that start in the
//                   block and where the last one completed, plus the first
//                   chunk failure (which does not depend on the state).
//   composition     tm_compose runs a file's summaries in order: each
//                   block's entry state and kept record count, the outcome
//                   the sequential reader reaches (the first failure, or the
//                   end-of-file rules of a short / full last block) and the
//                   valid end.  tm_compose_log applies the log rules to the
//                   files of one log.
//   records         tm_block_records finds the header offsets of the records
//                   that start in a block (no hashing); tm_record follows one
//                   record's chunks for its payload length and reads the two
//                   uvarints that name its owner.  A record's reader state
//                   "before" is recomputed from its header offset (tm_before).
//   replicas        tm_validate / tm_replay: tr_validate_record /
//                   tr_replay_record over a replica's record list.
//
// Every byte is read through a TanFile accessor at an offset compared with
// the file (or block) size first, as in drb_tanread.hpp.
#pragma once
#include "drb_tanread.hpp"

namespace drb {

constexpr uint32_t TM_NONE = 0xffffffffu;
constexpr uint32_t TM_KEYS = 16;  // logs per replica slot

// one file of a log; the files of log L = slot * 16 + key lie back to back
// in log order, the logs in L order
struct TmFile {
  uint64_t off, len;  // in the bytes
  uint32_t log;       // log number
  uint32_t blk0;      // its first block among all files' blocks
};

// what a block does to the reader, entered between records [0] or inside
// one [1]
struct TmBlock {
  uint32_t starts[2];    // records that start in the block
  uint32_t last_end[2];  // in-block offset behind the last record completed
                         // in it; TM_NONE
  uint32_t stop;         // the failing chunk's header, or where the block
                         // ran out
  uint8_t exit[2];       // the state behind the block (or at the failure)
  uint8_t fail;          // TR_ZEROED / TR_INVALID / TR_CRC; 0: none
  uint8_t tail_exact;    // the block ran out with end == n
};

struct TmFileOut {
  uint32_t outcome;  // TR_*: what the sequential reader ends the file with
  uint32_t records;  // complete records before it
  uint64_t valid_end;
};

// a log after its files' chunks (the statuses a record's owner adds come
// with the records: tm_owner_status)
struct TmLogOut {
  uint32_t status;  // TRS_OK, _TAIL_CUT, _EMPTY, _CORRUPT
  uint32_t log;     // the writer continues in this log ...
  uint64_t offset;  // ... here: behind the last kept record
  uint64_t records;
};

// a kept record: where its first chunk's header is, its payload length
struct TmRec {
  uint64_t hdr;
  uint32_t file, rlen;
};

DRB_TR_FN uint64_t tm_blocks(uint64_t len) {
  return (len + TR_BLOCK - 1) / TR_BLOCK;
}

// block b of f (b < tm_blocks(f.size)) as a file of its own
template <class In>
DRB_TR_FN TanFile<In> tm_block_file(const TanFile<In> &f, uint64_t b) {
  const uint64_t at = b * TR_BLOCK, left = f.size - at;
  return TanFile<In>{f.in, f.base + at, left < TR_BLOCK ? left : TR_BLOCK};
}

// one accepted chunk of type `type` seen in `state`: bit 0 a record starts
// with it, bit 1 a record completes with it (reader.next: wantFirst skips
// what is not FULL / FIRST; inside a record any chunk goes on, FULL / LAST
// end it -- tr_next_chunk's `last`)
DRB_TR_FN uint32_t tm_chunk(uint32_t &state, uint32_t type) {
  if (state == 0) {
    if (type == 1) return 3;
    if (type == 2) {
      state = 1;
      return 1;
    }
    return 0;
  }
  if (type == 1 || type == 4) {
    state = 0;
    return 2;
  }
  return 0;
}

// Pass A for one block.  tr_next_chunk on the one-block file, told to take
// every chunk; when it stops with room for a header left, the chunk there
// failed, else the block ran out (its INVALID / UNEXPECTED_EOF then only
// says so: what the end of a block means is the composition's to decide).
template <class In>
DRB_TR_FN TmBlock tm_summarize(const TanFile<In> &f, uint64_t b) {
  const TanFile<In> blk = tm_block_file(f, b);
  TmBlock s;
  uint32_t st[2] = {0, 1};
  s.starts[0] = s.starts[1] = 0;
  s.last_end[0] = s.last_end[1] = TM_NONE;
  s.fail = s.tail_exact = 0;
  TanWalk w;
  for (;;) {
    uint64_t begin;
    uint32_t clen;
    bool last;
    const int oc = tr_next_chunk(blk, w, false, true, &begin, &clen, &last);
    if (oc != TR_REC) {
      if (w.have_block && w.end + TR_HDR <= w.n)
        s.fail = (uint8_t)oc;
      else
        s.tail_exact = w.end == w.n;
      break;
    }
    const uint32_t type = blk.get(begin - 1);
    for (int e = 0; e < 2; ++e) {
      const uint32_t m = tm_chunk(st[e], type);
      if (m & 1) s.starts[e]++;
      if (m & 2) s.last_end[e] = w.end;
    }
  }
  s.stop = w.end;
  s.exit[0] = (uint8_t)st[0];
  s.exit[1] = (uint8_t)st[1];
  return s;
}

// A file's nb block summaries in order.  entry[b]: the state block b is
// entered in; cnt[b]: the records that start in it and complete before the
// file's end or first failure (a record left open there is not one: it is the
// last that started, in the block `open`).
DRB_TR_FN TmFileOut tm_compose(const TmBlock *sum, uint64_t nb, uint64_t size,
                               uint8_t *entry, uint32_t *cnt) {
  TmFileOut o;
  o.outcome = TR_EOF;
  o.records = 0;
  o.valid_end = 0;
  uint32_t state = 0;
  uint64_t open = ~0ull, b = 0;
  bool failed = false;
  for (; b < nb && !failed; ++b) {
    const TmBlock &s = sum[b];
    entry[b] = (uint8_t)state;
    cnt[b] = s.starts[state];
    o.records += s.starts[state];
    if (s.last_end[state] != TM_NONE)
      o.valid_end = b * TR_BLOCK + s.last_end[state];
    if (s.exit[state] == 0)
      open = ~0ull;
    else if (s.starts[state])
      open = b;
    state = s.exit[state];
    if (s.fail) {
      o.outcome = s.fail;
      failed = true;
    }
  }
  for (; b < nb; ++b) {  // behind the failure: not read
    entry[b] = 0;
    cnt[b] = 0;
  }
  if (!failed) {
    if (nb && size % TR_BLOCK)  // a short last block (record.go:267-279)
      o.outcome =
          state == 0 && sum[nb - 1].tail_exact ? TR_EOF : TR_INVALID;
    else  // io.ReadFull at the end of the file
      o.outcome = state == 0 ? TR_EOF : TR_UNEXPECTED_EOF;
  }
  if (state == 1 && open != ~0ull) {
    cnt[open]--;
    o.records--;
  }
  return o;
}

// The files [0, nf) of one log, in log order: rebuildLog's rules.  An
// invalid record in the last file cuts the log there; a CRC mismatch
// anywhere, or an invalid record in an earlier file, refuses it -- the files
// behind that are not read (their blocks yield no record).  fout: per file,
// or null.
DRB_TR_FN TmLogOut tm_compose_log(const TmFile *files, uint32_t nf,
                                  const TmBlock *sums, uint8_t *entry,
                                  uint32_t *cnt, TmFileOut *fout) {
  TmLogOut lo;
  lo.status = TRS_EMPTY;
  lo.log = 0;
  lo.offset = lo.records = 0;
  bool refused = false, cut = false;
  for (uint32_t k = 0; k < nf; ++k) {
    const TmFile &f = files[k];
    const uint64_t nb = tm_blocks(f.len);
    if (refused) {
      for (uint64_t b = 0; b < nb; ++b) entry[f.blk0 + b] = 0, cnt[f.blk0 + b] = 0;
      if (fout) fout[k] = TmFileOut{(uint32_t)TR_EOF, 0, 0};
      continue;
    }
    const TmFileOut o =
        tm_compose(sums + f.blk0, nb, f.len, entry + f.blk0, cnt + f.blk0);
    if (fout) fout[k] = o;
    lo.log = f.log;
    lo.offset = o.valid_end;
    lo.records += o.records;
    if (o.outcome == TR_EOF) continue;
    if (tr_invalid_record(o.outcome) && k + 1 == nf)
      cut = true;
    else
      refused = true;
  }
  if (nf) lo.status = refused ? TRS_CORRUPT : cut ? TRS_TAIL_CUT : TRS_OK;
  return lo;
}

// reader state in front of the chunk whose header is at `hdr` of a file of
// `size` bytes: a TanCur (or tr_walk_record) started from it reads that chunk
// first
DRB_TR_FN TanWalk tm_before(uint64_t hdr, uint64_t size) {
  TanWalk w;
  w.bstart = hdr / TR_BLOCK * TR_BLOCK;
  w.n = (uint32_t)(size - w.bstart < TR_BLOCK ? size - w.bstart : TR_BLOCK);
  w.pos = w.bstart + w.n;
  w.end = (uint32_t)(hdr - w.bstart);
  w.have_block = true;
  return w;
}

// Pass B for one block: emit(i, hdr) for the first cnt records that start in
// it, entered in state `entry` (no hashing: pass A accepted these chunks)
template <class In, class E>
DRB_TR_FN void tm_block_records(const TanFile<In> &f, uint64_t b,
                                uint32_t entry, uint32_t cnt, E &emit) {
  const TanFile<In> blk = tm_block_file(f, b);
  TanWalk w;
  uint32_t st = entry;
  for (uint32_t i = 0; i < cnt;) {
    uint64_t begin;
    uint32_t clen;
    bool last;
    if (tr_next_chunk(blk, w, false, false, &begin, &clen, &last) != TR_REC)
      return;  // (the summary counted cnt starts in front of this)
    if (tm_chunk(st, blk.get(begin - 1)) & 1)
      emit(i++, b * TR_BLOCK + begin - TR_HDR);
  }
}

// The record whose first chunk's header is at hdr: its payload length by
// its chunks (into the following blocks), its end, and the ShardID /
// ReplicaID its Update begins with.  TRS_OK, or TRS_CORRUPT: the ids do not
// parse (or the record is not one, or longer than 4 GiB).
template <class F>
DRB_TR_FN uint32_t tm_record(const F &f, uint64_t hdr, uint64_t *rlen,
                             uint64_t *end, uint64_t *shard,
                             uint64_t *replica) {
  const TanWalk before = tm_before(hdr, f.size);
  TanWalk w = before;
  if (tr_walk_record(f, w, false, rlen) != TR_REC || *rlen > 0xffffffffull)
    return TRS_CORRUPT;
  *end = tr_offset(w);
  TanCur<F> c(f, before, *rlen);
  if (!tr_uvarint(c, shard) || !tr_uvarint(c, replica)) return TRS_CORRUPT;
  return TRS_OK;
}

// whether a record of (shard, replica) belongs in log (slot, key) of an
// engine whose groups are ShardIDs [first_shard, first_shard + groups):
// TRS_OK and *g, or TRS_MISMATCH
DRB_TR_FN uint32_t tm_owner_status(uint64_t shard, uint64_t replica,
                                   uint64_t first_shard, uint64_t groups,
                                   uint32_t slot, uint32_t key, uint64_t *g) {
  if (replica != (uint64_t)slot + 1 || shard < first_shard ||
      shard - first_shard >= groups || shard % TM_KEYS != key)
    return TRS_MISMATCH;
  *g = shard - first_shard;
  return TRS_OK;
}

// record i of a replica: recs[order[i]], its file a TanFile over the bytes
struct TmRecRef {
  TanFile<TanFlatIn> f;
  TanWalk before;
  uint64_t rlen;
};
struct TmRecList {
  const uint8_t *bytes;
  const TmFile *files;
  const TmRec *recs;
  const uint32_t *order;  // the replica's record numbers, in log order
  DRB_TR_FN TmRecRef operator[](uint32_t i) const {
    const TmRec r = recs[order[i]];
    const TmFile fl = files[r.file];
    return TmRecRef{TanFile<TanFlatIn>{TanFlatIn{bytes}, fl.off, fl.len},
                    tm_before(r.hdr, fl.len), r.rlen};
  }
};

// Pass 1 for one replica of a multiplexed log: its n records (recs[i] a
// TmRecRef), all kept by the log.  plan.files / offset stay 0: the writer
// position is the log's.
template <class RL>
DRB_TR_FN TrPlan tm_validate(const RL &recs, uint32_t n, const TrLimits &lim) {
  TrPlan pl;
  TrReplay rp(lim.base_index);
  for (uint32_t i = 0; i < n; ++i) {
    const TmRecRef r = recs[i];
    const uint32_t st = tr_validate_record(r.f, r.before, r.rlen, lim, rp, pl);
    if (st != TRS_OK) {
      pl.status = st;
      return pl;
    }
  }
  tr_validate_finish(rp, lim, false, pl);
  return pl;
}

// Pass 2 for one replica whose plan is TRS_OK: as tr_replay
template <class RL, class P>
DRB_TR_FN bool tm_replay(const RL &recs, uint32_t n, const TrPlan &pl,
                         const TrLimits &lim, P &placer, uint64_t *applied) {
  TrReplay rp(lim.base_index);
  *applied = rp.applied;
  for (uint32_t i = 0; i < n; ++i) {
    const TmRecRef r = recs[i];
    if (!tr_replay_record(r.f, r.before, r.rlen, lim, rp, placer, applied))
      return false;
  }
  return tr_replay_finish(pl, rp, placer, applied);
}

}  // namespace drb
