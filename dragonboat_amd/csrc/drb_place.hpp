// drb_place.hpp -- MessageQueue.Add of the GPU inbox: how one delivered
// message enters a (group, sender, receiver) mailbox plane
// (include/drb_engine.h, drb_ingest_ex; record layout: drb_msg.hpp).  The
// one body behind both inbound drivers -- drb_ingest_ex, which gathers the
// planes' headers to the host and scatters the results, and k_ing_place
// (drb_ingest_wire), one lane per plane with direct stores.  It touches no
// memory: a driver loads what open() takes and stores what add() and
// close() return.  Plain C++ for the host and the device alike; also built
// under AddressSanitizer / UBSan by tests/test_place_rows.py.
#pragma once
#include "drb_layout.hpp"
#include "drb_msg.hpp"

namespace drb {

// the record add() made of one message
struct PlaneRec {
  uint32_t k;     // its position in the plane (rec_pos)
  uint4 c0, c1;   // the record
  bool own_term;  // MF_TERM_OTHER: `term` belongs in the rterm array at k
  uint64_t term;
};

struct Plane {
  uint4 cur;          // header: tag | quiesce, info, sender term
  uint64_t maxapp;    // max LogIndex + n of the Replicates (maxapp_valid)
  bool maxapp_valid;
  bool remote;        // placement C4: the sender slot lives on another rank
  uint64_t elo;       // remote: first index of the entry rows (0: none yet)

  // The stored header, max-append word and elo (remote planes) of the
  // plane; a header of another round's tag is nothing there yet this round.
  __host__ __device__ void open(uint4 hdr, uint64_t stored_maxapp,
                                uint64_t stored_elo, bool rm, uint32_t tag) {
    if (!tag_is(hdr.x, tag)) hdr = make_uint4(tag & MQ_TAG, 0, 0, 0);
    cur = hdr;
    maxapp = stored_maxapp;
    maxapp_valid = mi_nrep(hdr.y) > 0;
    remote = rm;
    // set by the round's first Replicate with entries placed here
    elo = rm && maxapp_valid ? stored_elo : 0;
  }

  // Whether the plane can hold a message of this shape; cmds_fit: none of
  // its entries' Cmds exceeds cmd_cap.  A message that does not fit sends
  // its receiver to the CPU path (DRB_FB_CAPACITY).
  __host__ __device__ bool fits(const View &v, uint32_t type, uint64_t n,
                                uint64_t log_index, bool cmds_fit) const {
    if (type == DRB_MSG_QUIESCE) return true;  // node-level: a header bit
    if (!cmds_fit || mi_count(cur.y) >= v.MB) return false;
    // handleFollowerPropose's message from another NodeHost: its entries
    // go to the sender's forward rows, one Propose per plane and round
    // (drb_config.forward_proposals)
    if (type == DRB_MSG_PROPOSE)
      return v.fwd_props && !remote && !(cur.y & MI_PROP) && n <= v.max_props;
    if (type != DRB_MSG_REPLICATE) return true;
    if (n > v.W) return false;  // (the window rows)
    if (!remote || !n) return true;
    // entry rows [elo, elo + E), elo set by the round's first Replicate
    // that carries entries (a commit-only one needs none)
    const uint64_t e0 = elo ? elo : log_index + 1;
    return log_index + 1 >= e0 && log_index + n - e0 < v.E;
  }

  // Takes a message that fits.  False: a Quiesce, which is the header's
  // MQ_QUIESCE bit and no record.  True: r is its record, to be stored at
  // position r.k; a Replicate's entry `index` then belongs in window row
  // `index` of the sender or, on a remote plane, in entry row index - elo.
  __host__ __device__ bool add(const View &v, const Msg &m, uint32_t to,
                               PlaneRec &r) {
    if (m.type == DRB_MSG_QUIESCE) {
      cur.x |= MQ_QUIESCE;
      return false;
    }
    const bool rep = m.type == DRB_MSG_REPLICATE;
    r.k = rec_pos(rep, rep ? mi_nrep(cur.y) : mi_noth(cur.y), v.MB);
    msg_encode(m, to, nullptr, r.c0, r.c1);
    // The sender's term is stored once per (sender, receiver, round) in the
    // header; a record whose term differs carries its own and makes the
    // receiver fall back (term gate, raft.go:1596-1609).  A pre-vote record
    // has a term of its own (r.term + 1 or the granted one, not the
    // sender's): it never seeds the header's term and always travels with
    // its own, as the step kernels' emit writes them.
    const bool zero = (r.c0.x & MF_TERM_ZERO) != 0;
    const bool pv = is_prevote_type(m.type);
    r.own_term = !zero && (pv || ((cur.y & MI_TERM) && q_hi(cur) != m.term));
    r.term = m.term;
    if (r.own_term) {
      r.c0.x |= MF_TERM_OTHER;
    } else if (!zero && !(cur.y & MI_TERM)) {
      cur.z = (uint32_t)m.term;
      cur.w = (uint32_t)(m.term >> 32);
    }
    const uint32_t inf = msg_info(m.type, zero, m.reject != 0, m.n) |
                         (r.own_term ? MI_TERM_OTHER : 0u);
    cur.y = (cur.y + (inf & MI_CNTS)) | (inf & ~MI_CNTS);
    if (rep) {
      const uint64_t ma = m.log_index + m.n;
      maxapp = maxapp_valid && maxapp > ma ? maxapp : ma;
      maxapp_valid = true;
      if (remote && m.n && !elo) elo = m.log_index + 1;
    }
    return true;
  }

  // Whether the receiver's inbox tag word gets this sender's byte, and the
  // byte (remote planes: the header's tag alone).
  __host__ __device__ bool close(uint8_t &byte) const {
    byte = tag_byte(cur.x, cur.y);  // (the header's tag is the round's)
    return !remote && (mi_count(cur.y) || (cur.x & MQ_QUIESCE));
  }
};

}  // namespace drb
