// drb_tanread.hpp -- the tan LogDB's read path: the record reader, the
// pb.Update decoder and the rules that turn a replica's log files back into
// its log, by one bounds-checked body for the host and the device.
//
//   record reader   internal/tan/record.go:163-311 (reader.nextChunk, next):
//                   32 KiB blocks, 7-byte legacy chunk headers {checksum u32,
//                   length u16, type u8}, FULL / FIRST / MIDDLE / LAST, zero
//                   padding where a header does not fit in the block, the
//                   checksum the low 32 bits of XXH64 over the type byte and
//                   the payload (crc.go:21-23).  Outcomes: io.EOF,
//                   ErrZeroedChunk, ErrInvalidChunk, ErrCRCMismatch,
//                   io.ErrUnexpectedEOF.
//   Update          raftpb/update.go:183-229 (Update.Unmarshal): uvarint
//                   ShardID and ReplicaID, a State behind a flag byte and a
//                   4-byte length (raftpb/state.go, protobuf fields 1-3), a
//                   4-byte entry count, each colfer Entry behind a 4-byte
//                   length (Entry.Unmarshal, raft_optimized.go:308-656), a
//                   Snapshot flag.
//   the logs        internal/tan/db.go:139-173, index.go:56-89,155-175,
//                   open.go:200-268: the State is that of the last record
//                   that has one; an Update whose first entry index is at or
//                   below the current last index overwrites from there; an
//                   invalid record (IsInvalidRecord, record.go:153-157:
//                   zeroed chunk, invalid chunk, unexpected EOF) in the LAST
//                   log ends that log there and the records before it stand
//                   (rebuildLog); a CRC mismatch anywhere, or an invalid
//                   record in an earlier log, is an error; entries are
//                   contiguous ("gap in indexes", db.go:243-249).
//
// Nothing here trusts a length from the file.  Every byte is read through
// TanFile::get / get64 at an offset the walker has compared with the file's
// size first: a chunk length that runs past its block, an entry length or
// count above what the record holds, a uvarint longer than 10 bytes and a
// record cut anywhere are outcomes (TR_INVALID ... TR_MALFORMED), never reads
// outside [0, size).
//
// A record is handled in two steps, as the reader does (a record's chunks are
// all read and checked before Unmarshal sees a byte): tr_walk_record walks
// and checks its chunks and leaves the walker behind it; a TanCur started
// from the walker's state BEFORE the record then yields the payload bytes in
// order, crossing chunk boundaries without hashing again.  Pass 2 of the
// device recovery (drb_recover.hpp) is that second step alone.
//
// The XXH64 constants and rounds are restated from drb_tan.hpp (the write
// path, __device__ only) under names of their own, so that header and the
// kernels compiled from it stay byte for byte what they were.
//
// Input goes through an accessor type In:
//   uint32_t get(uint64_t i)     byte i
//   uint64_t get64(uint64_t i)   bytes i .. i + 7, little endian
// TanFlatIn is a byte array.
//
// Plain C++ without __HIPCC__: no HIP runtime calls, no allocation, no
// recursion.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#ifdef __HIPCC__
#define DRB_TR_FN __host__ __device__ inline
#else
#define DRB_TR_FN inline
#endif

namespace drb {

constexpr uint32_t TR_BLOCK = 32768;  // blockSize (record.go:128)
constexpr uint32_t TR_HDR = 7;        // legacyHeaderSize (record.go:130)

// reader outcomes (the values of DRB_TAN_* in include/drb_engine.h); TR_REC
// is internal: a record was read
enum : int {
  TR_EOF = 0,
  TR_ZEROED = 1,
  TR_INVALID = 2,
  TR_CRC = 3,
  TR_UNEXPECTED_EOF = 4,
  TR_MALFORMED = 5,
  TR_REC = 6
};
// IsInvalidRecord (record.go:153-157)
DRB_TR_FN bool tr_invalid_record(int oc) {
  return oc == TR_ZEROED || oc == TR_INVALID || oc == TR_UNEXPECTED_EOF;
}

struct TanFlatIn {
  const uint8_t *p;
  DRB_TR_FN uint32_t get(uint64_t i) const { return p[i]; }
  DRB_TR_FN uint64_t get64(uint64_t i) const {
    uint64_t x;
    memcpy(&x, p + i, 8);  // (gfx950 and x86-64 are little endian)
    return x;
  }
};

// one log file: bytes [base, base + size) of the accessor
template <class In>
struct TanFile {
  In in;
  uint64_t base, size;
  DRB_TR_FN uint32_t get(uint64_t i) const { return in.get(base + i); }
  DRB_TR_FN uint64_t get64(uint64_t i) const { return in.get64(base + i); }
};

// ------------------------------------------------------------ XXH64
constexpr uint64_t TRP1 = 0x9E3779B185EBCA87ull;
constexpr uint64_t TRP2 = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t TRP3 = 0x165667B19E3779F9ull;
constexpr uint64_t TRP4 = 0x85EBCA77C2B2AE63ull;
constexpr uint64_t TRP5 = 0x27D4EB2F165667C5ull;

DRB_TR_FN uint64_t tr_rotl(uint64_t x, int r) {
  return (x << r) | (x >> (64 - r));
}
DRB_TR_FN uint64_t tr_round(uint64_t acc, uint64_t in) {
  return tr_rotl(acc + in * TRP2, 31) * TRP1;
}
DRB_TR_FN uint64_t tr_merge(uint64_t acc, uint64_t v) {
  return (acc ^ tr_round(0, v)) * TRP1 + TRP4;
}

// xxhash.Sum64 (cespare/xxhash/v2, seed 0) of bytes [off, off + n) of f;
// the caller has checked off + n <= f.size
template <class F>
DRB_TR_FN uint64_t tr_xxh64(const F &f, uint64_t off, uint64_t n) {
  uint64_t p = off, left = n, acc;
  if (n >= 32) {
    uint64_t v0 = TRP1 + TRP2, v1 = TRP2, v2 = 0, v3 = 0 - TRP1;
    for (; left >= 32; left -= 32, p += 32) {
      v0 = tr_round(v0, f.get64(p));
      v1 = tr_round(v1, f.get64(p + 8));
      v2 = tr_round(v2, f.get64(p + 16));
      v3 = tr_round(v3, f.get64(p + 24));
    }
    acc = tr_rotl(v0, 1) + tr_rotl(v1, 7) + tr_rotl(v2, 12) + tr_rotl(v3, 18);
    acc = tr_merge(acc, v0);
    acc = tr_merge(acc, v1);
    acc = tr_merge(acc, v2);
    acc = tr_merge(acc, v3);
  } else {
    acc = TRP5;
  }
  acc += n;
  for (; left >= 8; left -= 8, p += 8)
    acc = tr_rotl(acc ^ tr_round(0, f.get64(p)), 27) * TRP1 + TRP4;
  if (left >= 4) {
    uint64_t w = 0;
    for (uint32_t k = 0; k < 4; ++k) w |= (uint64_t)f.get(p + k) << (8 * k);
    acc = tr_rotl(acc ^ w * TRP1, 23) * TRP2 + TRP3;
    p += 4;
    left -= 4;
  }
  for (; left; --left, ++p)
    acc = tr_rotl(acc ^ (uint64_t)f.get(p) * TRP5, 11) * TRP1;
  acc ^= acc >> 33;
  acc *= TRP2;
  acc ^= acc >> 29;
  acc *= TRP3;
  acc ^= acc >> 32;
  return acc;
}

// ------------------------------------------------------------ chunk walker
// reader (record.go:163-199) over a file in memory: the block being read is
// bytes [bstart, bstart + n) of the file, `end` the position in it after the
// last chunk, `pos` the bytes handed out as blocks so far
struct TanWalk {
  uint64_t pos = 0, bstart = 0;
  uint32_t n = 0, end = 0;
  bool have_block = false;  // blockNum >= 0
};
// reader.offset (record.go:313-321)
DRB_TR_FN uint64_t tr_offset(const TanWalk &w) {
  return w.have_block ? w.bstart + w.end : 0;
}

// nextChunk (record.go:203-295).  TR_REC: the chunk's payload is bytes
// [*begin, *begin + *clen) of the file and *last says whether it ends its
// record; else the outcome.  `crc`: verify the checksum.
template <class F>
DRB_TR_FN int tr_next_chunk(const F &f, TanWalk &w, bool want_first, bool crc,
                            uint64_t *begin, uint32_t *clen, bool *last) {
  for (;;) {
    if (w.end + TR_HDR <= w.n) {
      const uint64_t a = w.bstart + w.end;  // a + 7 <= bstart + n <= size
      uint32_t checksum = 0;
      for (uint32_t k = 0; k < 4; ++k) checksum |= f.get(a + k) << (8 * k);
      const uint32_t length = f.get(a + 4) | (f.get(a + 5) << 8);
      const uint32_t type = f.get(a + 6);
      if (checksum == 0 && length == 0 && type == 0) {
        if (w.end + TR_HDR + 4 > w.n) {  // recyclableHeaderSize does not fit
          w.end = w.n;
          continue;
        }
        return TR_ZEROED;
      }
      // the recyclable types carry another log number or none: tan never
      // writes them (ErrInvalidChunk / EOF of a previous instance)
      if (type >= 5 && type <= 8) return TR_INVALID;
      const uint32_t b = w.end + TR_HDR;
      if (length > w.n - b) return TR_INVALID;  // runs past the block
      if (crc &&
          checksum != (uint32_t)tr_xxh64(f, a + 6, (uint64_t)length + 1))
        return TR_CRC;
      w.end = b + length;
      if (want_first && type != 1 && type != 2) continue;
      *begin = w.bstart + b;
      *clen = length;
      *last = type == 1 || type == 4;
      return TR_REC;
    }
    if (w.n < TR_BLOCK && w.have_block)
      return (!want_first || w.end != w.n) ? TR_INVALID : TR_EOF;
    if (w.pos >= f.size)  // io.ReadFull: io.EOF
      return want_first ? TR_EOF : TR_UNEXPECTED_EOF;
    w.bstart = w.pos;
    w.n = (uint32_t)(f.size - w.pos < TR_BLOCK ? f.size - w.pos : TR_BLOCK);
    w.pos += w.n;
    w.end = 0;
    w.have_block = true;
  }
}

// next + io.ReadAll of the record (record.go:300-311, db readers): every
// chunk of the next record, checked.  TR_REC: *rlen payload bytes, the
// walker stands behind the record.
template <class F>
DRB_TR_FN int tr_walk_record(const F &f, TanWalk &w, bool crc,
                             uint64_t *rlen) {
  uint64_t n = 0, begin;
  uint32_t clen;
  bool last = false, want_first = true;
  do {
    const int oc = tr_next_chunk(f, w, want_first, crc, &begin, &clen, &last);
    if (oc != TR_REC) return oc;
    n += clen;
    want_first = false;
  } while (!last);
  *rlen = n;
  return TR_REC;
}

// The payload of a record whose chunks tr_walk_record accepted, byte by
// byte: started from the walker's state before the record.  A read past the
// payload (`left` 0) or a chunk that no longer checks out sets `bad` and
// yields 0.
template <class F>
struct TanCur {
  const F *f;
  TanWalk w;
  uint64_t p = 0, cend = 0;  // the open chunk's unread bytes [p, cend)
  uint64_t left;             // payload bytes not yet taken
  bool first = true, last = false, bad = false;
  DRB_TR_FN TanCur(const F &file, const TanWalk &before, uint64_t rlen)
      : f(&file), w(before), left(rlen) {}
  DRB_TR_FN bool open() {  // the next chunk with bytes in it
    while (p == cend) {
      if (last) return false;
      uint64_t b;
      uint32_t n;
      if (tr_next_chunk(*f, w, first, false, &b, &n, &last) != TR_REC)
        return false;
      first = false;
      p = b;
      cend = b + n;
    }
    return true;
  }
  DRB_TR_FN uint32_t byte() {
    if (left == 0 || !open()) {
      bad = true;
      return 0;
    }
    left--;
    return f->get(p++);
  }
  DRB_TR_FN void skip(uint64_t n) {
    if (n > left) {
      bad = true;
      return;
    }
    left -= n;
    while (n) {
      if (!open()) {
        bad = true;
        return;
      }
      const uint64_t k = cend - p < n ? cend - p : n;
      p += k;
      n -= k;
    }
  }
};

// ------------------------------------------------------------ decoders
// binary.ReadUvarint (encoding/binary/varint.go): at most 10 bytes, the
// tenth at most 1
template <class C>
DRB_TR_FN bool tr_uvarint(C &c, uint64_t *out) {
  uint64_t x = 0;
  for (uint32_t k = 0; k < 10; ++k) {
    if (c.left == 0) return false;
    const uint32_t b = c.byte();
    if (b < 0x80) {
      if (k == 9 && b > 1) return false;
      *out = x | ((uint64_t)b << (7 * k));
      return !c.bad;
    }
    x |= (uint64_t)(b & 0x7f) << (7 * k);
  }
  return false;
}

template <class C>
DRB_TR_FN bool tr_le32(C &c, uint32_t *out) {
  if (c.left < 4) return false;
  uint32_t x = 0;
  for (uint32_t k = 0; k < 4; ++k) x |= c.byte() << (8 * k);
  *out = x;
  return !c.bad;
}

// pb.Entry without its Cmd (raftpb/entry.go:6-16)
struct TrEntry {
  uint64_t term, index, key, client_id, series_id, responded_to;
  uint32_t type, cmd_len;
};

// colfer u64 field body (raft_optimized.go:316-350) inside an entry of n
// bytes, i of them taken: a varint whose 9th byte is taken whole, or 8 bytes
// big endian after a 0x80-flagged header; a header byte always follows
template <class C>
DRB_TR_FN bool tr_colfer_u64(C &c, uint32_t n, uint32_t &i, bool flag,
                             uint64_t *v) {
  uint64_t x = 0;
  if (flag) {
    if (n - i < 9) return false;
    for (int k = 0; k < 8; ++k) x = (x << 8) | c.byte();
    i += 8;
    *v = x;
    return true;
  }
  for (uint32_t s = 0;; s += 7) {
    if (n - i < 2) return false;
    const uint64_t b = c.byte();
    i++;
    if (s == 56 || b < 0x80) {
      *v = x | (b << s);
      return true;
    }
    x |= (b & 0x7f) << s;
  }
}

// What receives an entry's Cmd: cmd(c, e) takes exactly e.cmd_len (>= 1)
// bytes from the cursor (c.byte() / c.skip()); the Cmd is the entry's last
// field, so e's other fields are complete.  TrSkipCmd keeps the first byte.
struct TrSkipCmd {
  uint32_t first_byte = 0;
  template <class C>
  DRB_TR_FN void cmd(C &c, const TrEntry &e) {
    first_byte = c.byte();
    c.skip(e.cmd_len - 1);
  }
};

// colfer Entry.Unmarshal (raft_optimized.go:308-656) of exactly n bytes of
// the cursor, n >= 1 and n <= c.left checked by the caller.  (Go accepts
// bytes after the 0x7f terminator; MarshalTo never writes any, and they are
// refused here.)
template <class C, class S>
DRB_TR_FN bool tr_entry(C &c, uint32_t n, TrEntry &e, S &sink) {
  e.term = e.index = e.key = e.client_id = e.series_id = e.responded_to = 0;
  e.type = e.cmd_len = 0;
  uint32_t i = 1;
  uint32_t h = c.byte();
  for (uint32_t tag = 0; tag < 7; ++tag) {
    if ((h & 0x7fu) != tag) continue;
    if (tag == 2) {  // Type: uint32 varint, 0x80 flag = negated
      uint64_t x = 0;
      for (uint32_t s = 0;; s += 7) {
        if (n - i < 2) return false;
        const uint64_t b = c.byte();
        i++;
        x |= (b & 0x7f) << s;
        if (b < 0x80) break;
        if (s > 28) return false;
      }
      e.type = (h & 0x80u) ? (uint32_t)(~(uint32_t)x + 1) : (uint32_t)x;
    } else {
      uint64_t x;
      if (!tr_colfer_u64(c, n, i, (h & 0x80u) != 0, &x)) return false;
      switch (tag) {
        case 0: e.term = x; break;
        case 1: e.index = x; break;
        case 3: e.key = x; break;
        case 4: e.client_id = x; break;
        case 5: e.series_id = x; break;
        default: e.responded_to = x; break;
      }
    }
    h = c.byte();  // i < n: the field bodies above leave a byte
    i++;
  }
  if (h == 7) {  // Cmd (raft_optimized.go:603-641)
    uint64_t x = 0;
    for (uint32_t s = 0;; s += 7) {
      if (i >= n) return false;
      const uint64_t b = c.byte();
      i++;
      x |= (b & 0x7f) << s;
      if (b < 0x80) break;
      if (s > 56) return false;
    }
    if (x > 16 * 1024 * 1024 || x >= n - i) return false;  // ColferSizeMax
    e.cmd_len = (uint32_t)x;
    if (e.cmd_len) sink.cmd(c, e);
    i += e.cmd_len;
    h = c.byte();
    i++;
  }
  return h == 0x7fu && i == n && !c.bad;
}

// the head of a pb.Update: everything before its entries
struct TrUpdate {
  uint64_t shard_id, replica_id, term, vote, commit;
  uint32_t has_state, n_entries;
};

// Update.Unmarshal (update.go:183-207) up to the entry count.  The State is
// protobuf fields 1-3 as varints (State.Unmarshal, raftpb/state.go), in any
// order; another field is refused (State.MarshalTo writes no other).  The
// count is checked against the bytes that follow: an entry takes at least
// its 4-byte length and a terminator.
template <class C>
DRB_TR_FN bool tr_update_head(C &c, TrUpdate &u) {
  u.term = u.vote = u.commit = 0;
  u.has_state = u.n_entries = 0;
  if (!tr_uvarint(c, &u.shard_id) || !tr_uvarint(c, &u.replica_id))
    return false;
  if (c.left == 0) return false;
  if (c.byte() != 0) {
    uint32_t l;
    if (!tr_le32(c, &l) || l > c.left) return false;
    const uint64_t stop = c.left - l;
    while (c.left > stop) {
      const uint32_t tag = c.byte();
      uint64_t x;
      // the value lies inside the State's length
      if (c.left <= stop || !tr_uvarint(c, &x) || c.left < stop) return false;
      if (tag == 0x08) u.term = x;
      else if (tag == 0x10) u.vote = x;
      else if (tag == 0x18) u.commit = x;
      else return false;
    }
    if (c.left != stop) return false;
    u.has_state = 1;
  }
  uint32_t cnt;
  if (!tr_le32(c, &cnt)) return false;
  if ((uint64_t)cnt * 5 > c.left) return false;
  u.n_entries = cnt;
  return !c.bad;
}

// the 4-byte length of the next entry, checked against the record
template <class C>
DRB_TR_FN bool tr_entry_len(C &c, uint32_t *n) {
  return tr_le32(c, n) && *n >= 1 && *n <= c.left;
}

// the Snapshot flag (update.go:221-227) and the record's end.  A Snapshot's
// bytes are skipped (*snapshot = true); bytes after the Update are refused.
template <class C>
DRB_TR_FN bool tr_update_tail(C &c, bool *snapshot) {
  *snapshot = false;
  if (c.left == 0) return false;
  if (c.byte() == 1) {
    uint32_t l;
    if (!tr_le32(c, &l) || l > c.left) return false;
    c.skip(l);
    *snapshot = true;
  }
  return c.left == 0 && !c.bad;
}

// Whether the rsm fast path applies an entry: prop_fast (drb_layout.hpp)
// restated for plain C++ (sessions: drb_config.session_slots > 0)
DRB_TR_FN bool tr_fast(const TrEntry &e, uint32_t first_byte, uint32_t snappy,
                       uint32_t sessions = 0) {
  if (e.type != 0 /*APPLICATION*/ && e.type != 2 /*ENCODED*/) return false;
  if (e.series_id != 0 && !sessions) return false;
  if (e.client_id == 0) return e.series_id == 0 && e.cmd_len == 0;
  if (e.series_id >= ~0ull - 1) return e.cmd_len == 0;
  if (e.type == 2 &&
      (e.cmd_len == 0 || !(first_byte == 0 || (snappy && first_byte == 2))))
    return false;
  return true;
}

// ------------------------------------------------------------ scan
// one record as drb_tan_scan reports it (drb_tan_scan_rec's fields)
struct TrScanRec {
  uint64_t offset, end, shard_id, replica_id, term, vote, commit, first_index,
      last_index;
  uint32_t has_state, n_entries;
};

// One record of the file: walks it (checksums), decodes it.  TR_REC, or the
// outcome that ends the file.  The walker stands behind the record.
template <class F>
DRB_TR_FN int tr_scan_record(const F &f, TanWalk &w, TrScanRec &r) {
  const TanWalk before = w;
  uint64_t rlen;
  r.offset = tr_offset(w);
  const int oc = tr_walk_record(f, w, true, &rlen);
  if (oc != TR_REC) return oc;
  r.end = tr_offset(w);
  TanCur<F> c(f, before, rlen);
  TrUpdate u;
  if (!tr_update_head(c, u)) return TR_MALFORMED;
  r.first_index = r.last_index = 0;
  for (uint32_t k = 0; k < u.n_entries; ++k) {
    uint32_t n;
    TrEntry e;
    TrSkipCmd sink;
    if (!tr_entry_len(c, &n) || !tr_entry(c, n, e, sink)) return TR_MALFORMED;
    if (k == 0) r.first_index = e.index;
    r.last_index = e.index;
  }
  bool snap;
  if (!tr_update_tail(c, &snap)) return TR_MALFORMED;
  r.shard_id = u.shard_id;
  r.replica_id = u.replica_id;
  r.term = u.term;
  r.vote = u.vote;
  r.commit = u.commit;
  r.has_state = u.has_state;
  r.n_entries = u.n_entries;
  return TR_REC;
}

// ------------------------------------------------------------ a replica
// statuses of a replica's recovery (DRB_REC_* in include/drb_engine.h)
enum : uint32_t {
  TRS_OK = 0,
  TRS_TAIL_CUT = 1,
  TRS_EMPTY = 2,
  TRS_CORRUPT = 3,
  TRS_MISMATCH = 4,
  TRS_GAP = 5,
  TRS_ENTRY_TYPE = 6,
  TRS_CAPACITY = 7,
  TRS_APPLY_STOPPED = 8,
  TRS_SNAPSHOT = 9
};

struct TrLimits {
  uint64_t shard_id, replica_id;
  uint64_t base_index;  // entries at or below it are skipped
  uint32_t cmd_cap, W;  // Cmd bytes and entries the window holds
  uint32_t snappy;      // drb_config.entry_compression
  uint32_t sessions = 0;  // drb_config.session_slots > 0
};

// what pass 1 decides about a replica; pass 2 replays `files` files, the
// last of them up to `offset`
struct TrPlan {
  uint32_t status = TRS_EMPTY;
  uint32_t files = 0;
  uint64_t offset = 0;
  uint64_t records = 0, entries = 0;  // kept records, their entries above base
  uint64_t term = 0, vote = 0, commit = 0, last_index = 0;
  // the highest index any kept record reached (>= last_index: an overwrite
  // may have cut a longer tail): what lies in the window ring is decided by
  // it, since every placed index takes slot index mod W
  uint64_t high_index = 0;
  // the last kept record has a State: what a db that wrote these records
  // holds in nodeStates (db.go:108-116), the next write's skip / sync input
  uint32_t state_stored = 0;
};

// The running state of a replica's replay, advanced record by record the
// same way by pass 1 (validation) and pass 2 (placement): the current last
// index under the overwrite rule, the last State, and the apply cursor of the
// rule "apply an occurrence only when it is final" -- while handling Update k
// with commit c_k (its State's, or the last one seen), first the pending
// (applied, min(c_k, first_k - 1)] is applied from the window, then each of
// its own entries i <= c_k as it is placed; an entry at or below a persisted
// commit is never overwritten by a later record.
// `high` is the highest index placed so far.  A placed index takes ring slot
// index mod W whether or not an overwrite cuts it off again later, so an
// entry still to be applied is intact exactly when nothing W or more above
// it was ever placed: pending entries are applied only while high - applied
// < W (else DRB_REC_CAPACITY, decided in pass 1), and the window that is
// left starts no lower than high + 1 - W.
struct TrReplay {
  uint64_t last, applied, high, commit = 0, term = 0, vote = 0;
  bool have_state = false;
  DRB_TR_FN explicit TrReplay(uint64_t base)
      : last(base), applied(base), high(base) {}
};

// One record of a replica in pass 1: the record whose chunks the caller has
// walked and checked (payload of rlen bytes, the reader's state `before` in
// front of it) is decoded and taken into the running state.  TRS_OK, or the
// status that refuses the replica.  The same body for a replica's own log
// files (tr_validate) and for its records in a multiplexed log
// (drb_tanmux.hpp).
template <class F>
DRB_TR_FN uint32_t tr_validate_record(const F &f, const TanWalk &before,
                                      uint64_t rlen, const TrLimits &lim,
                                      TrReplay &rp, TrPlan &pl) {
  TanCur<F> c(f, before, rlen);
  TrUpdate u;
  if (!tr_update_head(c, u)) return TRS_CORRUPT;
  if (u.shard_id != lim.shard_id || u.replica_id != lim.replica_id)
    return TRS_MISMATCH;
  const uint64_t ck = u.has_state ? u.commit : rp.commit;
  uint64_t first = 0, prev = 0;
  for (uint32_t j = 0; j < u.n_entries; ++j) {
    uint32_t n;
    TrEntry e;
    TrSkipCmd sink;
    if (!tr_entry_len(c, &n) || !tr_entry(c, n, e, sink)) return TRS_CORRUPT;
    if (j == 0) {
      first = e.index;
      // contiguity: an overwrite may start lower, never above last + 1
      if (first == 0 || first > rp.last + 1) return TRS_GAP;
      // an entry at or below a persisted commit is final
      if (first > lim.base_index && first <= rp.applied) return TRS_CORRUPT;
      // the pending span is applied from the window once this Update's
      // first entry is placed: that entry must not take a pending one's
      // place in the window
      const uint64_t hi = ck < first - 1 ? ck : first - 1;
      if (hi > rp.applied) {
        const uint64_t high = first > rp.high ? first : rp.high;
        if (high - rp.applied >= lim.W) return TRS_CAPACITY;
        rp.applied = hi;
      }
    } else if (e.index != prev + 1) {
      return TRS_GAP;
    }
    prev = e.index;
    if (e.index > lim.base_index) {
      if (!tr_fast(e, sink.first_byte, lim.snappy, lim.sessions))
        return TRS_ENTRY_TYPE;
      if (e.cmd_len > lim.cmd_cap) return TRS_CAPACITY;
      pl.entries++;
      if (e.index <= ck && e.index > rp.applied) rp.applied = e.index;
    }
  }
  bool snap;
  if (!tr_update_tail(c, &snap)) return TRS_CORRUPT;
  if (snap) return TRS_SNAPSHOT;
  if (u.n_entries) rp.last = prev > lim.base_index ? prev : lim.base_index;
  if (rp.last > rp.high) rp.high = rp.last;
  if (u.has_state) {
    rp.have_state = true;
    rp.term = u.term;
    rp.vote = u.vote;
    rp.commit = u.commit;
  }
  pl.records++;
  pl.state_stored = u.has_state;
  return TRS_OK;
}

// The end of pass 1: what the kept records amount to (pl.status and the
// final State), `cut` when the last log ended in an invalid record.
DRB_TR_FN void tr_validate_finish(const TrReplay &rp, const TrLimits &lim,
                                  bool cut, TrPlan &pl) {
  if (!rp.have_state) {  // ErrNoSavedLog
    pl.status = TRS_EMPTY;
    return;
  }
  // the State's commit lies in the log above the base
  if (rp.commit < lim.base_index) {
    pl.status = TRS_GAP;
    return;
  }
  if (rp.commit > rp.last) {
    pl.status = TRS_CORRUPT;
    return;
  }
  // the rest of (applied, commit] is applied from the window at the end
  if (rp.commit > rp.applied && rp.high - rp.applied >= lim.W) {
    pl.status = TRS_CAPACITY;
    return;
  }
  pl.term = rp.term;
  pl.vote = rp.vote;
  pl.commit = rp.commit;
  pl.last_index = rp.last;
  pl.high_index = rp.high;
  pl.status = cut ? TRS_TAIL_CUT : TRS_OK;
}

// Pass 1 for one replica: its files in log order (files[k] is file k, a
// TanFile; an array or anything indexable).  Decides status, kept prefix and
// final State without writing anything.
template <class FS>
DRB_TR_FN TrPlan tr_validate(const FS &files, uint32_t n_files,
                             const TrLimits &lim) {
  typedef typename std::decay<decltype(files[0])>::type F;
  TrPlan pl;
  TrReplay rp(lim.base_index);
  bool cut = false;
  for (uint32_t k = 0; k < n_files && !cut; ++k) {
    const F f = files[k];
    TanWalk w;
    pl.files = k + 1;
    pl.offset = 0;
    for (;;) {
      const TanWalk before = w;
      uint64_t rlen;
      const int oc = tr_walk_record(f, w, true, &rlen);
      if (oc == TR_EOF) break;
      if (oc != TR_REC) {
        if (tr_invalid_record(oc) && k + 1 == n_files) {
          cut = true;  // rebuildLog: the last log ends here
          break;
        }
        pl.status = TRS_CORRUPT;
        return pl;
      }
      const uint32_t st = tr_validate_record(f, before, rlen, lim, rp, pl);
      if (st != TRS_OK) {
        pl.status = st;
        return pl;
      }
      pl.offset = tr_offset(w);
    }
  }
  tr_validate_finish(rp, lim, cut, pl);
  return pl;
}

// One kept record in pass 2 (no checksums; pass 1 accepted it): every entry
// above the base handed to the placer, the committed ones applied.  false:
// the placer stopped the replay.
template <class F, class P>
DRB_TR_FN bool tr_replay_record(const F &f, const TanWalk &before,
                                uint64_t rlen, const TrLimits &lim,
                                TrReplay &rp, P &placer, uint64_t *applied) {
  TanCur<F> c(f, before, rlen);
  TrUpdate u;
  if (!tr_update_head(c, u)) return false;  // (pass 1 accepted it)
  const uint64_t ck = u.has_state ? u.commit : rp.commit;
  uint64_t prev = 0;
  for (uint32_t j = 0; j < u.n_entries; ++j) {
    uint32_t n;
    TrEntry e;
    if (!tr_entry_len(c, &n) || !tr_entry(c, n, e, placer)) return false;
    if (e.index > lim.base_index) placer.place(e);
    if (j == 0) {
      const uint64_t hi = ck < e.index - 1 ? ck : e.index - 1;
      while (rp.applied < hi) {
        if (!placer.apply(rp.applied + 1)) return false;
        *applied = ++rp.applied;
      }
    }
    prev = e.index;
    if (e.index > lim.base_index && e.index <= ck && e.index > rp.applied) {
      if (!placer.apply(e.index)) return false;
      *applied = rp.applied = e.index;
    }
  }
  if (u.n_entries) rp.last = prev > lim.base_index ? prev : lim.base_index;
  if (u.has_state) rp.commit = u.commit;
  return true;
}

// The end of pass 2: the rest of (applied, commit] from the window
template <class P>
DRB_TR_FN bool tr_replay_finish(const TrPlan &pl, TrReplay &rp, P &placer,
                                uint64_t *applied) {
  while (rp.applied < pl.commit) {
    if (!placer.apply(rp.applied + 1)) return false;
    *applied = ++rp.applied;
  }
  return true;
}

// Pass 2 for one replica whose plan is TRS_OK or TRS_TAIL_CUT: the kept
// records again, no checksums, every entry above the base handed to the
// placer P and the committed ones applied in index order, each once and in
// its final form:
//   template <class C> void cmd(C &c, const TrEntry &e)
//                            the Cmd's bytes (as TrSkipCmd; e.index says
//                            where it goes, at or below the base: nowhere)
//   void place(const TrEntry &e)   the entry's other fields, after its Cmd
//   bool apply(uint64_t index)     apply window entry `index`; false stops
//                                  the replay (tr_replay returns false)
// *applied receives the apply cursor (== plan.commit on success).
template <class FS, class P>
DRB_TR_FN bool tr_replay(const FS &files, const TrPlan &pl,
                         const TrLimits &lim, P &placer, uint64_t *applied) {
  typedef typename std::decay<decltype(files[0])>::type F;
  TrReplay rp(lim.base_index);
  *applied = rp.applied;
  for (uint32_t k = 0; k < pl.files; ++k) {
    const F f = files[k];
    TanWalk w;
    for (;;) {
      if (k + 1 == pl.files && tr_offset(w) >= pl.offset) break;
      const TanWalk before = w;
      uint64_t rlen;
      if (tr_walk_record(f, w, false, &rlen) != TR_REC) break;
      if (!tr_replay_record(f, before, rlen, lim, rp, placer, applied))
        return false;
    }
  }
  return tr_replay_finish(pl, rp, placer, applied);
}

}  // namespace drb
