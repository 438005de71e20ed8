// drb_snappy.hpp -- the payload of a Snappy-compressed EncodedEntry
// (Config.EntryCompressionType = Snappy), decoded on the host or on the
// device by one bounds-checked body.
//
// The Cmd of such an entry is the v0 header byte 0x02 (parseEncodedHeader,
// internal/rsm/encoded.go:119-125), then a Snappy block: the decoded length
// as a uvarint (getV0PayloadUncompressedSize, encoded.go:166-168), then
// literal and copy elements (golang/snappy v0.0.4 Decode):
//   tag & 3 == 0  literal, length - 1 in tag >> 2, or in the 1-4 bytes that
//                 follow when tag >> 2 is 60-63 (a long form of a short
//                 length is valid)
//   tag & 3 == 1  copy, length 4 + (tag >> 2 & 7), offset (tag >> 5) << 8 |
//                 next byte
//   tag & 3 == 2  copy, length 1 + (tag >> 2), 2-byte LE offset
//   tag & 3 == 3  copy, length 1 + (tag >> 2), 4-byte LE offset
// A copy may overlap its own output (offset < length: a run).
//
// Rejected, with no access outside [0, n) of the input or [0, cap) of the
// output: offset 0, an offset beyond the bytes produced so far, an element
// that runs past the input, output past the declared length, produced !=
// declared, declared 0, a uvarint that does not end inside the input or
// overflows 64 bits (binary.Uvarint), a declared length above cap.
//
// Input and output go through accessor types:
//   In:   uint32_t get(uint32_t i)            byte i of the Cmd, i < n
//   Out:  void put(uint32_t o, uint32_t b)    byte o, o = 0, 1, 2, ... in order
//         uint32_t get(uint32_t o, uint32_t done)  byte o < done, done the
//                                             count of bytes put so far
//         void finish(uint32_t n)             n bytes were put; called once
// SnapFlatIn / SnapFlatOut are byte arrays; SnapRowsIn / SnapRowsOut are rows
// of 16 B chunks a fixed stride apart -- the resident window's layout, chunk
// q of a lane's Cmd at base[q * G] -- which move 16 B at a time and keep the
// chunk being read or written in registers.
//
// Plain C++ without __HIPCC__: no HIP runtime calls, no allocation, no
// recursion.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DRB_SNAP_FN __host__ __device__ inline
#else
#define DRB_SNAP_FN inline
#endif

namespace drb {

struct SnapFlatIn {
  const uint8_t *p;
  DRB_SNAP_FN uint32_t get(uint32_t i) const { return p[i]; }
};

struct SnapFlatOut {
  uint8_t *p;
  DRB_SNAP_FN void put(uint32_t o, uint32_t b) { p[o] = (uint8_t)b; }
  DRB_SNAP_FN uint32_t get(uint32_t o, uint32_t) const { return p[o]; }
  DRB_SNAP_FN void finish(uint32_t) {}
};

// byte b (0..15) of a 16 B chunk {x, y, z, w}, by selects on values (a
// dynamically indexed array would live in scratch memory on the device)
template <class Q>
DRB_SNAP_FN uint32_t snap_q_byte(const Q &q, uint32_t b) {
  const uint32_t lo = (b & 4) ? q.y : q.x, hi = (b & 4) ? q.w : q.z;
  return (((b & 8) ? hi : lo) >> (8 * (b & 3))) & 0xffu;
}
template <class Q>
DRB_SNAP_FN void snap_q_or(Q &q, uint32_t b, uint32_t v) {
  const uint32_t x = v << (8 * (b & 3)), w = b >> 2;
  q.x |= w == 0 ? x : 0u;
  q.y |= w == 1 ? x : 0u;
  q.z |= w == 2 ? x : 0u;
  q.w |= w == 3 ? x : 0u;
}

// Q: a 16 B chunk with uint32_t members x, y, z, w (uint4 on the device)
template <class Q>
struct SnapRowsIn {
  const Q *base;    // chunk 0
  uint64_t stride;  // in chunks
  Q cur;
  uint32_t curq;
  DRB_SNAP_FN SnapRowsIn(const Q *b, uint64_t s)
      : base(b), stride(s), cur(), curq(~0u) {}
  DRB_SNAP_FN uint32_t get(uint32_t i) {
    if ((i >> 4) != curq) {
      curq = i >> 4;
      cur = base[(uint64_t)curq * stride];
    }
    return snap_q_byte(cur, i & 15);
  }
};

template <class Q>
struct SnapRowsOut {
  Q *base;
  uint64_t stride;
  Q acc;  // the chunk being filled (bytes not yet put are zero)
  Q rd;   // a finished chunk a copy reads from
  uint32_t rdq;
  DRB_SNAP_FN SnapRowsOut(Q *b, uint64_t s)
      : base(b), stride(s), acc(), rd(), rdq(~0u) {}
  DRB_SNAP_FN void put(uint32_t o, uint32_t b) {
    snap_q_or(acc, o & 15, b);
    if ((o & 15) == 15) {
      base[(uint64_t)(o >> 4) * stride] = acc;
      acc = Q();
    }
  }
  // o < the bytes put so far; chunks before the one being filled are final
  DRB_SNAP_FN uint32_t get(uint32_t o, uint32_t produced) {
    if ((o >> 4) == (produced >> 4)) return snap_q_byte(acc, o & 15);
    if ((o >> 4) != rdq) {
      rdq = o >> 4;
      rd = base[(uint64_t)rdq * stride];
    }
    return snap_q_byte(rd, o & 15);
  }
  // the last, partly filled chunk goes out with zeros after the payload, so
  // that no byte of an earlier, longer payload follows it inside the chunk
  DRB_SNAP_FN void finish(uint32_t n) {
    if (n & 15) base[(uint64_t)(n >> 4) * stride] = acc;
  }
};

// The block's declared length -- the decoded payload's, where the block is
// sound -- of the Cmd `in` of n bytes (binary.Uvarint at byte 1: at most 10
// bytes, the 10th at most 1); *next is the offset of the first element.
// 0: no length ends inside the Cmd, it overflows, or it is 0.
template <class In>
DRB_SNAP_FN uint64_t snappy_declared(In &in, uint32_t n, uint32_t *next) {
  uint64_t want = 0;
  uint32_t i = 1;
  for (uint32_t sh = 0;; sh += 7) {
    if (i >= n || sh > 63) return 0;
    const uint32_t b = in.get(i++);
    if (sh == 63 && b > 1) return 0;
    want |= (uint64_t)(b & 0x7f) << sh;
    if (!(b & 0x80)) break;
  }
  *next = i;
  return want;
}

// The Cmd `in` of n bytes (byte 0 the header, already checked to be 0x02)
// decoded into `out` of capacity cap bytes.  Returns 0 and the decoded
// length in *out_len, -1 for a corrupt block (`out` may then hold part of
// the payload), -3 for a declared length above cap (nothing is decoded).
template <class In, class Out>
DRB_SNAP_FN int snappy_decode(In &in, uint32_t n, Out &out, uint32_t cap,
                              uint32_t *out_len) {
  uint32_t i = 0;
  const uint64_t want = snappy_declared(in, n, &i);
  if (want == 0) return -1;
  if (want > cap) return -3;
  const uint32_t dlen = (uint32_t)want;
  uint32_t o = 0;
  while (i < n) {
    const uint32_t tag = in.get(i++);
    uint32_t len, off;
    if ((tag & 3) == 0) {
      len = tag >> 2;
      if (len >= 60) {
        const uint32_t nb = len - 59;
        if (nb > n - i) return -1;
        len = 0;
        for (uint32_t k = 0; k < nb; ++k) len |= in.get(i + k) << (8 * k);
        i += nb;
      }
      // (len + 1 would wrap at 0xffffffff: compared before the increment)
      if (len >= n - i || len >= dlen - o) return -1;
      len += 1;
      for (uint32_t k = 0; k < len; ++k, ++o) out.put(o, in.get(i + k));
      i += len;
      continue;
    }
    if ((tag & 3) == 1) {
      if (i >= n) return -1;
      len = 4 + ((tag >> 2) & 7);
      off = ((tag >> 5) << 8) | in.get(i++);
    } else if ((tag & 3) == 2) {
      if (n - i < 2) return -1;
      len = 1 + (tag >> 2);
      off = in.get(i) | (in.get(i + 1) << 8);
      i += 2;
    } else {
      if (n - i < 4) return -1;
      len = 1 + (tag >> 2);
      off = in.get(i) | (in.get(i + 1) << 8) | (in.get(i + 2) << 16) |
            (in.get(i + 3) << 24);
      i += 4;
    }
    if (off == 0 || off > o || len > dlen - o) return -1;
    for (uint32_t k = 0; k < len; ++k, ++o)
      out.put(o, out.get(o - off, o));
  }
  if (o != dlen) return -1;
  out.finish(o);
  *out_len = dlen;
  return 0;
}

// GetPayload (internal/rsm/encoded.go:55-66) of an entry's Cmd into out
// [0, cap).  Returns 0 and the payload's length, -1 for what the reference
// panics on or returns an error for (an unknown type or header, an empty
// encoded Cmd, a corrupt block), -3 for a payload, or a block's declared
// length, above cap.
DRB_SNAP_FN int payload_decode(uint32_t type, const uint8_t *cmd, size_t len,
                               uint8_t *out, size_t cap, size_t *out_len) {
  *out_len = 0;
  if (len > 0xffffffffu) return -1;
  size_t skip = 0;
  if (type == 2 /*ENCODED*/) {
    if (len == 0) return -1;
    const uint32_t h = cmd[0];
    if ((h & 0xf0) != 0 || (h & 1)) return -1;
    if ((h & 0x0e) == 2) {
      SnapFlatIn in = {cmd};
      SnapFlatOut o = {out};
      uint32_t dl = 0;
      const uint32_t c = cap > 0xffffffffu ? 0xffffffffu : (uint32_t)cap;
      const int rc = snappy_decode(in, (uint32_t)len, o, c, &dl);
      if (rc) return rc;
      *out_len = dl;
      return 0;
    }
    if ((h & 0x0e) != 0) return -1;
    skip = 1;
  } else if (type != 0 /*APPLICATION*/ && type != 1 /*CONFIG_CHANGE*/) {
    return -1;
  }
  if (len - skip > cap) return -3;
  for (size_t k = skip; k < len; ++k) out[k - skip] = cmd[k];
  *out_len = len - skip;
  return 0;
}

}  // namespace drb
