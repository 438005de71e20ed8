// drb_rows.hpp -- the two row formats entries travel in outside the step
// kernels, packed and unpacked in one place (drb_layout.hpp names the
// chunks).  Plain C++ for the host and the device alike; also built under
// AddressSanitizer / UBSan by tests/test_place_rows.py.
//
//   entry row     ENT_META chunks + C16 Cmd chunks (the window, a remote
//                 plane's entry rows)
//                   {term, key} {client_id, series_id}
//                   {responded_to, type u32, cmd_len u32}
//   proposal row  PROP_META chunks + C16 Cmd chunks (staged and forwarded
//                 proposals)
//                   {key, client_id} {series_id, responded_to}
//                   {type, cmd_len, prop_fast, 0}
//                 or, for a Cmd the row cannot hold, the capacity marker
//                   {type, ~0u, 1, 0}
//                 (the leader's pre-pass sends the group to the CPU path,
//                 DRB_FB_CAPACITY)
//   Cmd chunk c   bytes [16 c, 16 c + 16) of the Cmd, little endian words,
//                 zero past cmd_len
#pragma once
#include "drb_layout.hpp"
#include "drb_msg.hpp"

namespace drb {

// Cmd chunk c of the len bytes at p (p[i]: byte i; a pointer or a cursor)
template <class Src>
__host__ __device__ inline uint4 cmd_chunk(const Src &p, uint32_t len,
                                           uint32_t c) {
  uint32_t w[4] = {0, 0, 0, 0};
  for (uint32_t b = 0; b < 16 && c * 16 + b < len; ++b)
    w[b >> 2] |= (uint32_t)p[c * 16 + b] << (8 * (b & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__host__ __device__ inline void ent_pack(const drb_entry &en,
                                         uint4 *m /*ENT_META*/) {
  m[0] = pack2(en.term, en.key);
  m[1] = pack2(en.client_id, en.series_id);
  m[2] = pack2(en.responded_to, en.type | (uint64_t)en.cmd_len << 32);
}
// (index and cmd_off are the caller's: a row holds neither)
__host__ __device__ inline void ent_unpack(const uint4 *m, drb_entry &en) {
  en.term = q_lo(m[0]);
  en.key = q_hi(m[0]);
  en.client_id = q_lo(m[1]);
  en.series_id = q_hi(m[1]);
  en.responded_to = q_lo(m[2]);
  en.type = m[2].z;
  en.cmd_len = m[2].w;
}

// The proposal row's meta chunks of en, its Cmd at cmd.  readable: the
// cmd_len bytes lie inside what cmd points into.  Returns whether the row
// holds the Cmd (the caller then writes its chunks); else m[2] is the
// capacity marker and cmd is not read.
template <class Src>
__host__ __device__ inline bool prop_pack(const View &v, const drb_entry &en,
                                          const Src &cmd, bool readable,
                                          uint4 *m /*PROP_META*/) {
  m[0] = pack2(en.key, en.client_id);
  m[1] = pack2(en.series_id, en.responded_to);
  const bool held = readable && en.cmd_len <= v.C16 * 16;
  m[2] = held ? make_uint4(en.type, en.cmd_len,
                           prop_fast(en.type, en.client_id, en.series_id,
                                     en.cmd_len, en.cmd_len ? cmd[0] : 0u,
                                     v.snappy, v.sessions),
                           0)
              : make_uint4(en.type, ~0u, 1, 0);
  return held;
}
// (a proposal has no term and no index: the leader's append gives both)
__host__ __device__ inline void prop_unpack(const uint4 *m, drb_entry &en) {
  en.key = q_lo(m[0]);
  en.client_id = q_hi(m[0]);
  en.series_id = q_lo(m[1]);
  en.responded_to = q_hi(m[1]);
  en.type = m[2].x;
  en.cmd_len = m[2].y;
}

}  // namespace drb
