// drb_msgdec.hpp -- the decoder of one marshalled pb.Message, as
// drb_ingest_wire runs it on the bytes another NodeHost wrote: one
// bounds-checked body for the host and the device.
//
//   Message.Unmarshal   raftpb/raft_optimized.go:659-983 (gogo protobuf:
//                       varint fields 1-10 and 13, Entries 11, Snapshot 12,
//                       unknown fields through skipRaft, common.go:36-140)
//   Entry.unmarshal     raftpb/raft_optimized.go:308-656 (colfer: a header
//                       byte per field in tag order, 0x7f ends the entry)
//
// Nothing here trusts a length from the bytes: every index is compared
// with the message's length n before the byte is read, so a message cut or
// corrupted anywhere is an outcome (ING_BAD), never a read outside [0, n).
//
// What the decoder accepts is what the Go text accepts, not only what its
// marshallers emit:
//   - varints of up to 10 bytes, redundant continuation bytes included; the
//     bits a 10th byte holds above bit 63 are lost (shift >= 64 refuses,
//     :665-678);
//   - fields in any order, a scalar repeated (the last wins), scalars
//     between Entries elements;
//   - the field number is int32(wire >> 3) (:679): 2^32 + 1 is field 1,
//     what truncates to <= 0 is refused (:684);
//   - Type is an int32: the low 32 bits of its varint (:702);
//   - unknown fields of wire types 0, 1, 2 and 5 are skipped;
//   - in an entry, the Type and Cmd-length varints have no length limit:
//     the bits shifted past 32 / 64 are lost (:397-416, :608-626); a u64
//     varint's 9th byte is taken whole (:332); Type with the 0x80 header
//     flag is negated (:444); bytes after the 0x7f terminator inside the
//     Entries element are ignored (:645-650, called at :910);
//   - a Cmd is bounded by the bytes of its entry alone (ColferSizeMax is
//     8 TiB, :33; a message here is under 4 GiB);
//   - a zero-length Snapshot field is the empty Snapshot (Snapshot.Unmarshal
//     of no bytes sets nothing).
// A Snapshot that is not the canonical empty one (nor zero-length) makes
// the message ING_SNAPSHOT -- the CPU path's, which decodes the Snapshot
// itself -- but only once the rest of the message has been scanned: what
// follows it malformed refuses the batch as Go does (:940-943 then the
// loop goes on).
//
// Refused on purpose although Go accepts it (the frame is ING_BAD, never a
// different decoded value; no Go marshaller emits it):
//   - MD_REFUSE_GROUP: an unknown field of wire type 3 (a protobuf group,
//     skipRaft common.go:98-129).  raft.proto has no groups.
//
// Plain C++ without __HIPCC__: no HIP runtime calls, no allocation, no
// recursion.  tests/native/msgdecode.cpp builds it with g++ under
// AddressSanitizer / UBSan.
#pragma once
#include <stdint.h>

#include "../../include/drb_engine.h"

#ifdef __HIPCC__
#define DRB_MD_FN __host__ __device__ inline
#else
#define DRB_MD_FN inline
#endif

namespace drb {

// one decoded pb.Message (raftpb/message.go:6-20) of an ingested stream
struct DecMsg {
  uint64_t shard, from, to, term, log_term, log_index, commit, hint,
      hint_high;
  uint64_t ent0;   // its first entry in the decoded entry array
  uint32_t type, reject, n_ent, err;  // err: ING_*
};
constexpr uint32_t ING_OK = 0, ING_BAD = 1, ING_SNAPSHOT = 2, ING_BIG = 3;

// A lane's byte cursor over the uploaded stream: one load per byte, which
// hit the L1 (a 16 B register window measured 2-4 % slower on the C3
// plane, profiles/r04_ingest)
struct Bytes {
  const uint8_t *p;
  DRB_MD_FN explicit Bytes(const uint8_t *d) : p(d) {}
  DRB_MD_FN uint32_t operator[](uint64_t i) const { return p[i]; }
};

// (every index below is from the message's first byte; d_entry's from the
// entry's, at offset e0)
template <class B>
DRB_MD_FN bool d_varint(B &d, uint32_t n, uint32_t &i, uint64_t &v) {
  v = 0;
  for (uint32_t s = 0; s < 70; s += 7) {
    if (i >= n) return false;
    const uint32_t b = d[i++];
    v |= (uint64_t)(b & 0x7fu) << s;
    if (b < 0x80u) return true;
  }
  return false;
}

// skipRaft (raft.pb.go): an unknown field
template <class B>
DRB_MD_FN bool d_skip(B &d, uint32_t n, uint32_t &i, uint64_t wire) {
  uint64_t x;
  switch (wire & 7) {
    case 0: return d_varint(d, n, i, x);
    case 1: i += 8; return i <= n;
    case 2:
      if (!d_varint(d, n, i, x) || x > n - i) return false;
      i += (uint32_t)x;
      return true;
    case 5: i += 4; return i <= n;
    // 3: MD_REFUSE_GROUP (above); 4, 6, 7: refused by Go too (:681,
    // common.go:135)
    default: return false;
  }
}

// colfer u64 field body (raft_optimized.go:316-350): varint whose 9th
// byte is taken whole, or 8 bytes big endian after a 0x80-flagged tag
template <class B>
DRB_MD_FN bool d_colfer_u64(B &d, uint32_t e0, uint32_t n, uint32_t &i,
                            bool flag, uint64_t &v) {
  if (flag) {
    if (i + 8 >= n) return false;
    v = 0;
    for (int k = 0; k < 8; ++k) v = (v << 8) | d[e0 + i + k];
    i += 8;
    return true;
  }
  v = 0;
  for (uint32_t s = 0;; s += 7) {
    if (i + 1 >= n) return false;
    const uint64_t b = d[e0 + i++];
    if (s == 56 || b < 0x80) {
      v |= b << s;
      return true;
    }
    v |= (b & 0x7f) << s;
  }
}

// colfer Entry.Unmarshal (raft_optimized.go:308-656) of the n bytes at e0;
// cmd_off is the Cmd's offset from e0
template <class B>
DRB_MD_FN bool d_entry(B &d, uint32_t e0, uint32_t n, drb_entry &e) {
  e.term = e.index = e.key = e.client_id = e.series_id = e.responded_to = 0;
  e.type = e.cmd_len = 0;
  e.cmd_off = 0;
  if (n == 0) return false;
  uint32_t i = 1;
  uint32_t h = d[e0];
  for (uint32_t tag = 0; tag < 7; ++tag) {
    if ((h & 0x7fu) != tag || h == 0x7fu) continue;
    if (tag == 2) {  // Type: uint32 varint, 0x80 flag = negated
      // (no length limit, :397-416: a uint32 shifted by 32 or more is 0 in
      // Go; s stops growing there, so it cannot wrap in a long varint)
      uint32_t x = 0;
      for (uint32_t s = 0;; s = s < 32 ? s + 7 : s) {
        if (i + 1 >= n) return false;
        const uint32_t b = d[e0 + i++];
        if (s < 32) x |= (b & 0x7fu) << s;
        if (b < 0x80u) break;
      }
      e.type = (h & 0x80u) ? ~x + 1 : x;
    } else {
      uint64_t x;
      if (!d_colfer_u64(d, e0, n, i, (h & 0x80u) != 0, x)) return false;
      switch (tag) {
        case 0: e.term = x; break;
        case 1: e.index = x; break;
        case 3: e.key = x; break;
        case 4: e.client_id = x; break;
        case 5: e.series_id = x; break;
        default: e.responded_to = x; break;
      }
    }
    h = d[e0 + i++];
  }
  if (h == 7) {  // Cmd (raft_optimized.go:603-641)
    // (the length varint has no limit either: Go's uint loses the bits
    // shifted past 64)
    uint64_t x = 0;
    for (uint32_t s = 0;; s = s < 64 ? s + 7 : s) {
      if (i >= n) return false;
      const uint64_t b = d[e0 + i++];
      if (s < 64) x |= (b & 0x7f) << s;
      if (b < 0x80) break;
    }
    // the Cmd and the header byte after it lie inside the entry (:632-636;
    // ColferSizeMax, 8 TiB, is above every n)
    if (x >= n - i) return false;
    e.cmd_off = i;
    e.cmd_len = (uint32_t)x;
    i += (uint32_t)x;
    h = d[e0 + i++];
  }
  // (what follows the terminator inside the element is ignored, :645-650)
  return h == 0x7fu;
}

// the empty pb.Snapshot every fast-path message embeds (snapshot.go:72-150
// with every field zero), byte k
DRB_MD_FN uint32_t md_empty_snapshot(uint32_t k) {
  static constexpr uint8_t s[24] = {
      0x12, 0, 0x18, 0, 0x20, 0, 0x28, 0, 0x32, 2, 0x08, 0,
      0x48, 0, 0x50, 0, 0x58, 0, 0x60, 0, 0x68, 0, 0x70, 0};
  return s[k];
}

// Message.Unmarshal (raft_optimized.go:659-983).  ents == nullptr: count
// the entries only.  Returns ING_*; big when a Cmd exceeds cmd_cap.
// While the scan runs, m.reject also carries its two flags (MD_F_*): a word
// of their own cost the kernels registers (k_ing_decode a wave of
// occupancy).  They are taken out again before an ING_OK / ING_SNAPSHOT
// return; the record of an ING_BAD message is never delivered.
constexpr uint32_t MD_F_REJECT = 1, MD_F_SNAPSHOT = 2, MD_F_BIG = 4;
DRB_MD_FN uint32_t d_message(const uint8_t *msg, uint32_t n, DecMsg &m,
                             drb_entry *ents, uint64_t base,
                             uint32_t cmd_cap, bool &big) {
  Bytes d(msg);
  m.shard = m.from = m.to = m.term = m.log_term = m.log_index = m.commit = 0;
  m.hint = m.hint_high = 0;
  m.type = m.reject = m.n_ent = 0;
  uint32_t i = 0;
  while (i < n) {
    uint64_t wire, v;
    if (!d_varint(d, n, i, wire)) return ING_BAD;
    // fieldNum := int32(wire >> 3), refused when <= 0 (:679-686)
    const int32_t field = (int32_t)(uint32_t)(wire >> 3);
    const uint32_t wt = (uint32_t)(wire & 7);
    if (field <= 0) return ING_BAD;
    if ((field >= 1 && field <= 10) || field == 13) {
      if (wt != 0 || !d_varint(d, n, i, v)) return ING_BAD;
      switch (field) {
        case 1: m.type = (uint32_t)v; break;
        case 2: m.to = v; break;
        case 3: m.from = v; break;
        case 4: m.shard = v; break;
        case 5: m.term = v; break;
        case 6: m.log_term = v; break;
        case 7: m.log_index = v; break;
        case 8: m.commit = v; break;
        case 9:
          m.reject = (m.reject & ~MD_F_REJECT) | (v != 0 ? MD_F_REJECT : 0u);
          break;
        case 10: m.hint = v; break;
        default: m.hint_high = v; break;
      }
    } else if (field == 11 || field == 12) {
      uint64_t l;
      if (wt != 2 || !d_varint(d, n, i, l) || l > n - i) return ING_BAD;
      if (field == 11) {
        drb_entry e;
        if (!d_entry(d, i, (uint32_t)l, e)) return ING_BAD;
        if (e.cmd_len > cmd_cap) m.reject |= MD_F_BIG;
        if (ents) {
          e.cmd_off += base + i;  // the Cmd's offset in the stream
          ents[m.n_ent] = e;
        }
        m.n_ent++;
      } else {
        // (no bytes: Snapshot.Unmarshal sets nothing, the empty Snapshot)
        bool empty = l == 24;
        for (uint32_t k = 0; empty && k < 24; ++k)
          empty = d[i + k] == md_empty_snapshot(k);
        // InstallSnapshot: the CPU path's, once the rest has been scanned
        if (!empty && l != 0) m.reject |= MD_F_SNAPSHOT;
      }
      i += (uint32_t)l;
    } else if (!d_skip(d, n, i, wire)) {
      return ING_BAD;
    }
  }
  const uint32_t fl = m.reject;
  m.reject = fl & MD_F_REJECT;
  if (fl & MD_F_BIG) big = true;
  return (fl & MD_F_SNAPSHOT) ? ING_SNAPSHOT : ING_OK;
}

}  // namespace drb
