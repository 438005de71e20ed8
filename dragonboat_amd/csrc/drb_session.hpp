// drb_session.hpp -- the client session table of a replica (the rsm side of
// dragonboat's at-most-once proposals), decided, committed, imported and
// exported by one body on the host and on the device.
//
// Reference (internal/rsm): handleEntry (statemachine.go:935-969) sends a
// session-managed entry (ClientID != 0, raftpb/raft.go:87-128) to
//   registerSession   SeriesID = SeriesIDForRegister (MaxUint64 - 1), empty Cmd
//                     (client/session.pb.go:27-38): RegisterClientID
//                     (sessionmanager.go:54-67) adds the session and returns
//                     Result{Value: clientID}; a known client gets the empty
//                     Result, which ApplyUpdate takes as rejected
//   unregisterSession SeriesIDForUnregister (MaxUint64), empty Cmd:
//                     UnregisterClientID (:72-83) deletes, Value = clientID;
//                     unknown: rejected
//   update            (:1057-1103) anything else with SeriesID != 0:
//                     ClientRegistered (:86-95), else rejected; then
//                     UpdateRespondedTo -> Session.clearTo (session.go:88-103:
//                     history keys are always above RespondedUpTo, so both of
//                     its branches are "drop every key <= to, RespondedUpTo =
//                     max"); hasResponded(series) -> ignored; a getResponse
//                     hit -> the cached Result, the state machine untouched;
//                     else sm.Update and addResponse(series, result)
// Every getSession hit and every add moves the session to the most recently
// used end (lrusession.go); OrderedDo / save walk least recently used first
// (lrusession.go:93-120).
//
// The table of a replica: S sessions of 2 + H chunks of 16 B
//   chunk 0       {client_id u64, responded_up_to u64}; client_id 0: free
//                 (NotSessionManagedClientID never registers)
//   chunk 1       {last-use stamp u64, history occupancy mask u32, 0}
//   chunk 2 + h   {series_id u64, value u64} of history slot h < H
// The stamp is monotonic per replica (the entry index plus SESS_MAX_SLOTS
// on an apply; the position in the list on an import): its one contract is
// the order of the export.  A cleared history bit leaves its chunk behind;
// the mask alone says what is held.
//
// Decide first, store after: sess_decide loads and stores nothing;
// sess_commit stores what the plan says.  A `full` plan, or an update whose
// state machine call then fails, leaves the table as it was.
//
// The table goes through an accessor type T:
//   uint64_t lo(uint32_t c)         the low 8 bytes of chunk c
//   Q get(uint32_t c)               chunk c (Q: uint32_t members x, y, z, w)
//   void put(uint32_t c, Q q)
// SessFlat is an array of chunks; SessRows has the chunks a stride apart
// (the device layout [R][S][2 + H][G], group innermost: stride G).
//
// Plain C++ without __HIPCC__: no HIP runtime calls, no allocation.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define DRB_SESS_FN __host__ __device__ inline
// (the slot arrays stay in registers only when their loops are unrolled)
#define DRB_SESS_UNROLL _Pragma("unroll")
#else
#define DRB_SESS_FN inline
#define DRB_SESS_UNROLL
#endif

namespace drb {

constexpr uint32_t SESS_MAX_SLOTS = 16;    // drb_config.session_slots
constexpr uint32_t SESS_MAX_HISTORY = 8;   // drb_config.session_history
constexpr uint64_t SESS_SERIES_REGISTER = ~0ull - 1;  // SeriesIDForRegister
constexpr uint64_t SESS_SERIES_UNREGISTER = ~0ull;    // SeriesIDForUnregister
// a Result.Value the table and the outcome ring hold: below 2^62
constexpr uint64_t SESS_VALUE_MAX = (1ull << 62) - 1;

enum : uint32_t {
  SESS_REGISTERED = 0,     // value = client
  SESS_REGISTER_DUP = 1,   // rejected
  SESS_UNREGISTERED = 2,   // value = client
  SESS_UNREGISTER_UNKNOWN = 3,  // rejected
  SESS_UNKNOWN_CLIENT = 4,      // rejected
  SESS_RESPONDED = 5,      // ignored
  SESS_CACHED = 6,         // value from the history
  SESS_UPDATE = 7,         // the caller updates the SM, then commits
  SESS_FULL = 8            // no free session / history slot
};

// per-entry apply codes (the outcome ring's top 2 bits, drb_apply_result)
enum : uint32_t { SESS_CODE_APPLIED = 0, SESS_CODE_REJECTED = 1,
                  SESS_CODE_IGNORED = 2 };

DRB_SESS_FN uint32_t sess_code(uint32_t outcome) {
  return outcome == SESS_REGISTER_DUP || outcome == SESS_UNREGISTER_UNKNOWN ||
                 outcome == SESS_UNKNOWN_CLIENT
             ? SESS_CODE_REJECTED
             : (outcome == SESS_RESPONDED ? SESS_CODE_IGNORED
                                          : SESS_CODE_APPLIED);
}

// a 16 B chunk on the host (uint4 on the device)
struct SessQ {
  uint32_t x, y, z, w;
};

template <class Q>
DRB_SESS_FN Q sess_q(uint64_t lo, uint64_t hi) {
  Q q;
  q.x = (uint32_t)lo;
  q.y = (uint32_t)(lo >> 32);
  q.z = (uint32_t)hi;
  q.w = (uint32_t)(hi >> 32);
  return q;
}
template <class Q>
DRB_SESS_FN uint64_t sess_lo(const Q &q) {
  return (uint64_t)q.x | ((uint64_t)q.y << 32);
}
template <class Q>
DRB_SESS_FN uint64_t sess_hi(const Q &q) {
  return (uint64_t)q.z | ((uint64_t)q.w << 32);
}

template <class Q>
struct SessFlat {
  typedef Q chunk;
  Q *p;
  DRB_SESS_FN uint64_t lo(uint32_t c) const { return sess_lo(p[c]); }
  DRB_SESS_FN Q get(uint32_t c) const { return p[c]; }
  DRB_SESS_FN void put(uint32_t c, const Q &q) { p[c] = q; }
};

template <class Q>
struct SessRows {
  typedef Q chunk;
  Q *base;          // chunk 0
  uint64_t stride;  // in chunks
  DRB_SESS_FN uint64_t lo(uint32_t c) const {
    // (an 8-byte load: the lookup reads only the client ids)
    const Q *q = base + (uint64_t)c * stride;
    return (uint64_t)q->x | ((uint64_t)q->y << 32);
  }
  DRB_SESS_FN Q get(uint32_t c) const { return base[(uint64_t)c * stride]; }
  DRB_SESS_FN void put(uint32_t c, const Q &q) {
    base[(uint64_t)c * stride] = q;
  }
};

// what sess_decide found: the outcome, the session slot it concerns (the
// hit, or the free slot a register takes), the history slot an update's
// response takes, and the session's RespondedUpTo and history mask behind
// the entry's own clearTo
struct SessPlan {
  uint32_t outcome, slot, hslot, mask;
  uint64_t responded;
  uint64_t value;  // registered / unregistered: client; cached: the Result
};

// The outcome of one session-managed entry (series != 0) against the table;
// nothing is stored.
template <class T>
DRB_SESS_FN SessPlan sess_decide(const T &t, uint32_t S, uint32_t H,
                                 uint64_t client, uint64_t series,
                                 uint64_t responded_to, uint32_t cmd_len) {
  typedef typename T::chunk Q;
  SessPlan p;
  p.outcome = SESS_FULL;
  p.slot = p.hslot = p.mask = 0;
  p.responded = p.value = 0;
  const uint32_t CH = 2 + H;
  // the lookup: every slot's client id, the loads issued back to back
  uint64_t ids[SESS_MAX_SLOTS];
  DRB_SESS_UNROLL
  for (uint32_t s = 0; s < SESS_MAX_SLOTS; ++s)
    ids[s] = s < S ? t.lo(s * CH) : 0;
  uint32_t hit = SESS_MAX_SLOTS, fre = SESS_MAX_SLOTS;
  DRB_SESS_UNROLL
  for (int s = (int)SESS_MAX_SLOTS - 1; s >= 0; --s) {
    if ((uint32_t)s < S && ids[s] == client) hit = (uint32_t)s;
    if ((uint32_t)s < S && ids[s] == 0) fre = (uint32_t)s;
  }
  const bool found = hit < SESS_MAX_SLOTS;
  Q c0 = Q(), c1 = Q();
  if (found) {
    c0 = t.get(hit * CH);
    c1 = t.get(hit * CH + 1);
    p.slot = hit;
    p.responded = sess_hi(c0);
    p.mask = c1.z;
  }
  if (cmd_len == 0 && series == SESS_SERIES_REGISTER) {
    if (found) {
      p.outcome = SESS_REGISTER_DUP;
    } else if (fre < SESS_MAX_SLOTS) {
      p.outcome = SESS_REGISTERED;
      p.slot = fre;
      p.value = client;
    }
    return p;
  }
  if (cmd_len == 0 && series == SESS_SERIES_UNREGISTER) {
    p.outcome = found ? SESS_UNREGISTERED : SESS_UNREGISTER_UNKNOWN;
    if (found) p.value = client;
    return p;
  }
  if (!found) {
    p.outcome = SESS_UNKNOWN_CLIENT;
    return p;
  }
  // the history, in one trip; then clearTo(responded_to) on the copies
  Q hs[SESS_MAX_HISTORY];
  DRB_SESS_UNROLL
  for (uint32_t h = 0; h < SESS_MAX_HISTORY; ++h)
    hs[h] = h < H ? t.get(hit * CH + 2 + h) : Q();
  if (responded_to > p.responded) {
    p.responded = responded_to;
  DRB_SESS_UNROLL
    for (uint32_t h = 0; h < SESS_MAX_HISTORY; ++h)
      if (h < H && sess_lo(hs[h]) <= responded_to) p.mask &= ~(1u << h);
  }
  if (series <= p.responded) {
    p.outcome = SESS_RESPONDED;
    return p;
  }
  uint32_t freeh = SESS_MAX_HISTORY;
  bool cached = false;
  DRB_SESS_UNROLL
  for (int h = (int)SESS_MAX_HISTORY - 1; h >= 0; --h) {
    if ((uint32_t)h >= H) continue;
    if (!((p.mask >> h) & 1u)) {
      freeh = (uint32_t)h;
    } else if (sess_lo(hs[h]) == series) {
      cached = true;
      p.value = sess_hi(hs[h]);
    }
  }
  if (cached) {
    p.outcome = SESS_CACHED;
  } else if (freeh < SESS_MAX_HISTORY) {
    p.outcome = SESS_UPDATE;
    p.hslot = freeh;
  }
  return p;
}

// The stores of a decided entry (not SESS_FULL).  stamp: above every stamp
// in the table.  value: an update's Result.Value (<= SESS_VALUE_MAX).
template <class T>
DRB_SESS_FN void sess_commit(T &t, uint32_t H, const SessPlan &p,
                             uint64_t client, uint64_t series, uint64_t stamp,
                             uint64_t value) {
  typedef typename T::chunk Q;
  const uint32_t b = p.slot * (2 + H);
  switch (p.outcome) {
    case SESS_REGISTERED:
      t.put(b, sess_q<Q>(client, 0));
      t.put(b + 1, sess_q<Q>(stamp, 0));
      break;
    case SESS_REGISTER_DUP:  // the getSession hit is a use
      t.put(b + 1, sess_q<Q>(stamp, p.mask));
      break;
    case SESS_UNREGISTERED:
      t.put(b, sess_q<Q>(0, 0));
      t.put(b + 1, sess_q<Q>(0, 0));
      break;
    case SESS_RESPONDED:
    case SESS_CACHED:
      t.put(b, sess_q<Q>(client, p.responded));
      t.put(b + 1, sess_q<Q>(stamp, p.mask));
      break;
    case SESS_UPDATE:
      t.put(b + 2 + p.hslot, sess_q<Q>(series, value));
      t.put(b, sess_q<Q>(client, p.responded));
      t.put(b + 1, sess_q<Q>(stamp, p.mask | (1u << p.hslot)));
      break;
    default:  // unregister-unknown, unknown-client: getSession missed
      break;
  }
}

// ------------------------------------------------------------ hand-over
// drb_session_rec / drb_session_resp (include/drb_engine.h), restated so
// that the header stands alone
struct SessRec {
  uint64_t client_id, responded_up_to;
  uint32_t n_history, first_history;
};
struct SessResp {
  uint64_t series_id, value;
};

// The table's sessions least recently used first (lrusession.save's order),
// each one's responses by ascending series.  *n / *n_hist: the full counts;
// false when a cap is too small (nothing past a cap is written).
template <class T>
DRB_SESS_FN bool sess_export(const T &t, uint32_t S, uint32_t H, SessRec *recs,
                             size_t cap, SessResp *hist, size_t hist_cap,
                             size_t *n, size_t *n_hist) {
  typedef typename T::chunk Q;
  const uint32_t CH = 2 + H;
  size_t nr = 0, nh = 0;
  uint64_t after = 0;  // stamps are distinct: walk them in ascending order
  bool first = true;
  for (;;) {
    uint32_t best = S;
    uint64_t bs = 0;
    for (uint32_t s = 0; s < S; ++s) {
      if (t.lo(s * CH) == 0) continue;
      const uint64_t st = sess_lo(t.get(s * CH + 1));
      if (!first && st <= after) continue;
      if (best == S || st < bs) {
        best = s;
        bs = st;
      }
    }
    if (best == S) break;
    first = false;
    after = bs;
    const Q c0 = t.get(best * CH), c1 = t.get(best * CH + 1);
    SessRec r;
    r.client_id = sess_lo(c0);
    r.responded_up_to = sess_hi(c0);
    r.n_history = 0;
    r.first_history = (uint32_t)nh;
    uint64_t prev = 0;  // series are distinct and above RespondedUpTo >= 0
    for (;;) {
      uint32_t bh = H;
      uint64_t bser = 0;
      for (uint32_t h = 0; h < H; ++h) {
        if (!((c1.z >> h) & 1u)) continue;
        const uint64_t ser = sess_lo(t.get(best * CH + 2 + h));
        if (ser <= prev) continue;
        if (bh == H || ser < bser) {
          bh = h;
          bser = ser;
        }
      }
      if (bh == H) break;
      prev = bser;
      if (nh < hist_cap) {
        hist[nh].series_id = bser;
        hist[nh].value = sess_hi(t.get(best * CH + 2 + bh));
      }
      ++nh;
      ++r.n_history;
    }
    if (nr < cap) recs[nr] = r;
    ++nr;
  }
  *n = nr;
  *n_hist = nh;
  return nr <= cap && nh <= hist_cap;
}

// Replaces the table with `n` sessions in sess_export's order.  false, with
// the table untouched: more than S sessions, more than H responses in one, a
// value above SESS_VALUE_MAX, a zero or repeated client_id, a zero or
// repeated series_id in a session or one at or below its responded_up_to
// (clearTo would have dropped it), responses outside [0, n_hist).
template <class T>
DRB_SESS_FN bool sess_import(T &t, uint32_t S, uint32_t H, const SessRec *recs,
                             size_t n, const SessResp *hist, size_t n_hist) {
  typedef typename T::chunk Q;
  if (n > S) return false;
  for (size_t i = 0; i < n; ++i) {
    const SessRec &r = recs[i];
    if (r.client_id == 0 || r.n_history > H) return false;
    if ((size_t)r.first_history > n_hist ||
        (size_t)r.n_history > n_hist - r.first_history)
      return false;
    for (size_t j = 0; j < i; ++j)
      if (recs[j].client_id == r.client_id) return false;
    for (uint32_t h = 0; h < r.n_history; ++h) {
      const SessResp &x = hist[r.first_history + h];
      if (x.value > SESS_VALUE_MAX || x.series_id <= r.responded_up_to)
        return false;
      for (uint32_t k = 0; k < h; ++k)
        if (hist[r.first_history + k].series_id == x.series_id) return false;
    }
  }
  const uint32_t CH = 2 + H;
  for (uint32_t s = 0; s < S; ++s) {
    if (s >= n) {
      for (uint32_t c = 0; c < CH; ++c) t.put(s * CH + c, sess_q<Q>(0, 0));
      continue;
    }
    const SessRec &r = recs[s];
    t.put(s * CH, sess_q<Q>(r.client_id, r.responded_up_to));
    t.put(s * CH + 1,
          sess_q<Q>((uint64_t)s, r.n_history ? (1u << r.n_history) - 1u : 0u));
    for (uint32_t h = 0; h < H; ++h)
      t.put(s * CH + 2 + h,
            h < r.n_history ? sess_q<Q>(hist[r.first_history + h].series_id,
                                        hist[r.first_history + h].value)
                            : sess_q<Q>(0, 0));
  }
  return true;
}

}  // namespace drb
