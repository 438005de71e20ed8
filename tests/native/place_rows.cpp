// place_rows.cpp -- the placement rule (drb_place.hpp) and the row codec
// (drb_rows.hpp) on the CPU, with no engine and no device.
//
// Placement, on a View with MB=4, W=8, E=4, C16=2, max_props=2, fwd_props=1:
// the header reset of a stale tag, the record positions (Replicates up from
// 0, the others down from MB - 1), the capacities (records, one Propose per
// plane, max_props, forward rows, the window, a remote plane's entry rows,
// cmd_cap), elo and the max-append word, the header term and the records
// that carry their own, the inbox tag byte, and that every record decodes
// (msg_decode) to the message put in.  Rows: entry and proposal rows round
// trip at Cmd lengths 0, 1, 15, 16, 17, 32 with zero bytes past the Cmd, a
// Cmd of 33 bytes gives the capacity marker, the fast word is prop_fast's.
// The expected values are written out from drb_msg.hpp's and
// include/drb_engine.h's descriptions.
//
// Built by tests/test_place_rows.py with -fsanitize=address,undefined.
// Prints "ok <checks>" and exits 0, or the first mismatch and 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../../dragonboat_amd/csrc/drb_place.hpp"
#include "../../dragonboat_amd/csrc/drb_rows.hpp"

using namespace drb;

static unsigned long long g_checked = 0;

#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                               \
    }                                                        \
    ++g_checked;                                             \
  } while (0)

static bool eq4(uint4 q, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
  return q.x == x && q.y == y && q.z == z && q.w == w;
}

static View limits() {
  View v;
  memset(&v, 0, sizeof(v));
  v.G = 1;
  v.R = 3;
  v.MB = 4;
  v.W = 8;
  v.E = 4;
  v.C16 = 2;
  v.max_props = 2;
  v.fwd_props = 1;
  return v;
}

static const uint32_t TAG = 6;

static Plane fresh(bool remote = false) {
  Plane p;
  // another round's header, with records, a term and stale words beside it
  p.open(make_uint4(TAG - 1, 2 | MI_TERM, 9, 0), 77, 55, remote, TAG);
  return p;
}

static Msg msg(uint32_t type, uint64_t term) {
  Msg m;
  memset(&m, 0, sizeof(m));
  m.type = type;
  m.term = term;
  return m;
}
static Msg replicate(uint64_t term, uint64_t log_index, uint32_t n,
                     uint64_t log_term, uint64_t commit) {
  Msg m = msg(DRB_MSG_REPLICATE, term);
  m.log_index = log_index;
  m.n = n;
  m.log_term = log_term;
  m.commit = commit;
  return m;
}
static Msg heartbeat(uint64_t term, uint64_t commit = 40) {
  Msg m = msg(DRB_MSG_HEARTBEAT, term);
  m.commit = commit;
  m.hint = 0x1111222233334444ull;
  m.hint_high = 0x5555666677778888ull;
  return m;
}

// m fits, is added, and its record decodes to m with the header term or
// the record's own
static PlaneRec add(const View &v, Plane &p, const Msg &m) {
  CHECK(p.fits(v, m.type, m.n, m.log_index, true));
  PlaneRec r;
  memset(&r, 0xa5, sizeof(r));
  CHECK(p.add(v, m, 1, r));
  CHECK(r.k < v.MB);
  CHECK(((r.c0.x & MF_TERM_OTHER) != 0) == r.own_term);
  uint64_t lo = 0, hi = 0;
  const Msg d =
      msg_decode(r.c0, r.c1, r.own_term ? r.term : q_hi(p.cur), lo, hi);
  CHECK(d.type == m.type && d.reject == m.reject && d.n == m.n);
  CHECK(d.term == m.term);
  CHECK(d.log_index == m.log_index && d.log_term == m.log_term);
  CHECK(d.commit == m.commit);
  CHECK(d.hint == m.hint && d.hint_high == m.hint_high);
  return r;
}

static void open_cases() {
  // a stale tag opens as an empty header with the current tag
  Plane p = fresh();
  CHECK(eq4(p.cur, TAG, 0, 0, 0));
  CHECK(!p.maxapp_valid && p.elo == 0 && !p.remote);
  p.open(make_uint4(TAG - 1, 1, 9, 0), 77, 55, true, 0x80000000u | TAG);
  CHECK(eq4(p.cur, TAG, 0, 0, 0));  // the tag is 31 bits
  CHECK(!p.maxapp_valid && p.elo == 0 && p.remote);
  // this round's header stays, Quiesce bit included; elo is a remote
  // plane's, and only once a Replicate was placed
  p.open(make_uint4(MQ_QUIESCE | TAG, 1 | MI_TERM, 9, 1), 77, 55, true, TAG);
  CHECK(eq4(p.cur, MQ_QUIESCE | TAG, 1 | MI_TERM, 9, 1));
  CHECK(p.maxapp_valid && p.maxapp == 77 && p.elo == 55);
  p.open(make_uint4(TAG, 1 | MI_TERM, 9, 1), 77, 55, false, TAG);
  CHECK(p.maxapp_valid && p.maxapp == 77 && p.elo == 0);
  p.open(make_uint4(TAG, (1u << MI_NOTH) | MI_TERM, 9, 1), 77, 55, true, TAG);
  CHECK(!p.maxapp_valid && p.elo == 0);
}

static void position_cases() {
  const View v = limits();
  Plane p = fresh();
  // one Replicate and three Heartbeats fill the plane: positions 0; 3, 2, 1
  CHECK(add(v, p, replicate(3, 10, 2, 3, 9)).k == 0);
  CHECK(add(v, p, heartbeat(3)).k == 3);
  CHECK(add(v, p, heartbeat(3)).k == 2);
  CHECK(add(v, p, heartbeat(3)).k == 1);
  // counts, "carries the term", and a leader leaves the fast path for both
  // types; the term once in the header; max-append = LogIndex + n
  CHECK(eq4(p.cur, TAG, 1u | (3u << 5) | MI_OFF_LEADER | MI_TERM, 3, 0));
  CHECK(p.maxapp_valid && p.maxapp == 12);
  // a fifth does not fit
  CHECK(!p.fits(v, DRB_MSG_HEARTBEAT, 0, 0, true));
  CHECK(!p.fits(v, DRB_MSG_REPLICATE, 0, 12, true));
  // a Quiesce still does, and takes no record
  CHECK(p.fits(v, DRB_MSG_QUIESCE, 0, 0, true));
  PlaneRec r;
  CHECK(!p.add(v, msg(DRB_MSG_QUIESCE, 0), 1, r));
  CHECK(eq4(p.cur, MQ_QUIESCE | TAG,
            1u | (3u << 5) | MI_OFF_LEADER | MI_TERM, 3, 0));
  // Replicates alone count up
  Plane q = fresh();
  for (uint32_t k = 0; k < 4; ++k)
    CHECK(add(v, q, replicate(3, 10 + k, 1, 2, 9)).k == k);
  CHECK(!q.fits(v, DRB_MSG_REPLICATE, 1, 14, true));
}

static void propose_cases() {
  View v = limits();
  Msg pr = msg(DRB_MSG_PROPOSE, 0);
  pr.n = 2;
  Plane p = fresh();
  const PlaneRec r = add(v, p, pr);
  CHECK(r.k == 3 && !r.own_term && (r.c0.x & MF_TERM_ZERO));
  CHECK((p.cur.y & MI_PROP) && mi_nprop(p.cur.y) == 2);
  CHECK(!p.fits(v, DRB_MSG_PROPOSE, 1, 0, true));  // a second one
  CHECK(p.fits(v, DRB_MSG_HEARTBEAT, 0, 0, true));
  Plane q = fresh();
  CHECK(q.fits(v, DRB_MSG_PROPOSE, 2, 0, true));
  CHECK(!q.fits(v, DRB_MSG_PROPOSE, 3, 0, true));   // max_props
  CHECK(!q.fits(v, DRB_MSG_PROPOSE, 1, 0, false));  // a Cmd over cmd_cap
  CHECK(!q.fits(v, DRB_MSG_PROPOSE, 1ull << 32, 0, true));
  Plane rm = fresh(true);
  CHECK(!rm.fits(v, DRB_MSG_PROPOSE, 1, 0, true));  // a remote plane
  v.fwd_props = 0;
  CHECK(!q.fits(v, DRB_MSG_PROPOSE, 1, 0, true));   // no forward rows
}

static void replicate_cases() {
  const View v = limits();
  Plane p = fresh();
  CHECK(p.fits(v, DRB_MSG_REPLICATE, 8, 100, true));
  CHECK(!p.fits(v, DRB_MSG_REPLICATE, 9, 100, true));   // n > W
  CHECK(!p.fits(v, DRB_MSG_REPLICATE, 1, 100, false));  // cmd_cap
  // a local plane has no entry rows to run out of
  add(v, p, replicate(3, 20, 2, 3, 9));
  CHECK(p.elo == 0);
  CHECK(p.fits(v, DRB_MSG_REPLICATE, 8, 2, true));

  Plane r = fresh(true);
  CHECK(!r.fits(v, DRB_MSG_REPLICATE, 5, 20, true));  // rows [21, 25)
  CHECK(r.fits(v, DRB_MSG_REPLICATE, 4, 20, true));
  CHECK(r.elo == 0);  // (asking changes nothing)
  // a commit-only Replicate needs no rows and sets no elo
  CHECK(add(v, r, replicate(3, 5, 0, 3, 5)).k == 0);
  CHECK(r.elo == 0 && r.maxapp_valid && r.maxapp == 5);
  // the first with entries sets elo = LogIndex + 1
  CHECK(add(v, r, replicate(3, 20, 2, 3, 9)).k == 1);
  CHECK(r.elo == 21 && r.maxapp == 22);
  CHECK(!r.fits(v, DRB_MSG_REPLICATE, 1, 19, true));  // LogIndex + 1 < elo
  CHECK(!r.fits(v, DRB_MSG_REPLICATE, 3, 22, true));  // 22 + 3 - 21 >= E
  CHECK(r.fits(v, DRB_MSG_REPLICATE, 2, 22, true));
  CHECK(r.fits(v, DRB_MSG_REPLICATE, 0, 3, true));    // commit-only
  CHECK(add(v, r, replicate(3, 3, 0, 3, 3)).k == 2);
  CHECK(r.elo == 21 && r.maxapp == 22);  // the maximum, elo left alone
  CHECK(add(v, r, replicate(3, 22, 2, 3, 9)).k == 3);
  CHECK(r.elo == 21 && r.maxapp == 24);
  CHECK(mi_nrep(r.cur.y) == 4 && mi_noth(r.cur.y) == 0);
}

static void term_cases() {
  const View v = limits();
  // the first record with a term seeds the header and carries none
  Plane p = fresh();
  PlaneRec r = add(v, p, heartbeat(5));
  CHECK(!r.own_term && p.cur.z == 5 && p.cur.w == 0);
  CHECK((p.cur.y & MI_TERM) && !(p.cur.y & MI_TERM_OTHER));
  // another term: its own, reported at its own position
  r = add(v, p, heartbeat((7ull << 32) | 1));
  CHECK(r.own_term && r.term == ((7ull << 32) | 1) && r.k == 2);
  CHECK((p.cur.y & MI_TERM_OTHER) && p.cur.z == 5 && p.cur.w == 0);
  r = add(v, p, heartbeat(5));
  CHECK(!r.own_term && r.k == 1);
  // a wide term is seeded whole
  Plane w = fresh();
  add(v, w, heartbeat((9ull << 32) | 2));
  CHECK(w.cur.z == 2 && w.cur.w == 9);
  // a RequestPreVote never seeds and always carries its own term
  Plane q = fresh();
  Msg pv = msg(DRB_MSG_REQUEST_PREVOTE, 8);
  pv.log_index = 30;
  pv.log_term = 7;
  pv.hint = 2;
  r = add(v, q, pv);
  CHECK(r.own_term && r.term == 8 && r.k == 3);
  CHECK(q.cur.z == 0 && q.cur.w == 0 && (q.cur.y & MI_TERM_OTHER));
  Plane s = fresh();
  add(v, s, heartbeat(8));
  r = add(v, s, pv);  // the header's term is the same: still its own
  CHECK(r.own_term && r.term == 8 && s.cur.z == 8);
  r = add(v, s, msg(DRB_MSG_REQUEST_PREVOTE_RESP, 9));
  CHECK(r.own_term && r.term == 9 && s.cur.z == 8);
  // a request type with term 0: MF_TERM_ZERO, seeds nothing
  Plane z = fresh();
  Msg ri = msg(DRB_MSG_READ_INDEX, 0);
  ri.hint = 11;
  ri.hint_high = 12;
  r = add(v, z, ri);
  CHECK((r.c0.x & MF_TERM_ZERO) && !r.own_term);
  CHECK(z.cur.z == 0 && z.cur.w == 0 && !(z.cur.y & (MI_TERM | MI_TERM_OTHER)));
  r = add(v, z, heartbeat(4));  // the header's term was still free
  CHECK(!r.own_term && z.cur.z == 4);
  r = add(v, z, ri);  // and a term-0 request differs from no header term
  CHECK(!r.own_term && !(z.cur.y & MI_TERM_OTHER));
}

static void tag_cases() {
  const View v = limits();
  uint8_t b = 0;
  Plane p = fresh();
  CHECK(!p.close(b));  // nothing placed
  add(v, p, heartbeat(3));
  CHECK(p.close(b) && b == TAG);
  add(v, p, replicate(3, 10, 0, 3, 9));
  CHECK(p.close(b) && b == (TAG | 0x80u));
  Plane q = fresh();
  Msg rr = msg(DRB_MSG_REPLICATE_RESP, 3);
  rr.log_index = 12;
  add(v, q, rr);
  CHECK(q.close(b) && b == (TAG | 0x80u));
  rr.reject = 1;
  rr.hint = 10;
  add(v, q, rr);
  CHECK(q.cur.y & MI_REJECT);
  Plane f = fresh();
  Msg pr = msg(DRB_MSG_PROPOSE, 0);
  pr.n = 1;
  add(v, f, pr);
  CHECK(f.close(b) && b == (TAG | 0x80u));
  // a Quiesce alone is due a byte, and is not heavy
  Plane z = fresh();
  PlaneRec r;
  CHECK(!z.add(v, msg(DRB_MSG_QUIESCE, 0), 1, r));
  CHECK(z.close(b) && b == TAG);
  // the byte is the round mod 128
  Plane t;
  t.open(make_uint4(0, 0, 0, 0), 0, 0, false, 0x12b4);
  add(v, t, heartbeat(3));
  CHECK(t.close(b) && b == 0x34);
  // a remote plane has the header's tag alone
  Plane rm = fresh(true);
  add(v, rm, replicate(3, 10, 1, 3, 9));
  CHECK(!rm.close(b));
}

// a byte source that is no pointer
struct Cursor {
  const uint8_t *p;
  uint32_t operator[](uint64_t i) const { return p[i]; }
};

static void row_cases() {
  const View v = limits();
  uint8_t pool[64];
  for (uint32_t i = 0; i < sizeof(pool); ++i) pool[i] = (uint8_t)(0x81 + i);
  const uint32_t lens[] = {0, 1, 15, 16, 17, 32};
  for (uint32_t len : lens) {
    drb_entry en;
    memset(&en, 0, sizeof(en));
    en.term = 0x0102030405060708ull;
    en.key = 0x1112131415161718ull;
    en.client_id = 0x2122232425262728ull;
    en.series_id = 0x3132333435363738ull;
    en.responded_to = 0x4142434445464748ull;
    en.type = DRB_ENTRY_ENCODED;
    en.cmd_len = len;
    const uint8_t *cmd = pool + 5;
    // the Cmd chunks: the bytes in order, zero past cmd_len
    uint8_t got[32];
    for (uint32_t c = 0; c < v.C16; ++c) {
      const uint4 q = cmd_chunk(cmd, len, c);
      const uint4 q2 = cmd_chunk(Cursor{cmd}, len, c);
      CHECK(eq4(q2, q.x, q.y, q.z, q.w));
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
      for (uint32_t b = 0; b < 16; ++b)
        got[c * 16 + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
    for (uint32_t b = 0; b < 32; ++b) CHECK(got[b] == (b < len ? cmd[b] : 0));
    // the entry row: {term, key} {client, series} {responded_to, type, len}
    uint4 m[ENT_META];
    ent_pack(en, m);
    CHECK(eq4(m[0], 0x05060708u, 0x01020304u, 0x15161718u, 0x11121314u));
    CHECK(eq4(m[1], 0x25262728u, 0x21222324u, 0x35363738u, 0x31323334u));
    CHECK(eq4(m[2], 0x45464748u, 0x41424344u, DRB_ENTRY_ENCODED, len));
    drb_entry back;
    memset(&back, 0xee, sizeof(back));
    ent_unpack(m, back);
    back.index = en.index;
    back.cmd_off = en.cmd_off;
    CHECK(memcmp(&back, &en, sizeof(en)) == 0);
    // the proposal row: {key, client} {series, responded_to}
    // {type, len, fast, 0}
    for (uint64_t series : {0x3132333435363738ull, 0ull}) {
      en.series_id = series;
      const uint32_t fast = prop_fast(en.type, en.client_id, en.series_id, len,
                                      len ? cmd[0] : 0u, v.snappy);
      uint4 pm[PROP_META];
      CHECK(prop_pack(v, en, cmd, true, pm));
      CHECK(eq4(pm[0], 0x15161718u, 0x11121314u, 0x25262728u, 0x21222324u));
      CHECK(eq4(pm[1], (uint32_t)series, (uint32_t)(series >> 32), 0x45464748u,
                0x41424344u));
      CHECK(eq4(pm[2], DRB_ENTRY_ENCODED, len, fast, 0));
      uint4 pc[PROP_META];
      CHECK(prop_pack(v, en, Cursor{cmd}, true, pc));
      CHECK(memcmp(pc, pm, sizeof(pm)) == 0);
      memset(&back, 0, sizeof(back));
      prop_unpack(pm, back);
      drb_entry want = en;
      want.term = 0;
      CHECK(memcmp(&back, &want, sizeof(want)) == 0);
    }
  }
  // the fast word is prop_fast's: both values occur
  drb_entry en;
  memset(&en, 0, sizeof(en));
  en.type = DRB_ENTRY_ENCODED;
  en.client_id = 9;
  en.cmd_len = 4;
  uint8_t zero_hdr[4] = {0, 1, 2, 3}, other_hdr[4] = {7, 1, 2, 3};
  uint4 pm[PROP_META];
  CHECK(prop_pack(v, en, zero_hdr, true, pm) && pm[2].z == 1);
  CHECK(prop_pack(v, en, other_hdr, true, pm) && pm[2].z == 0);
  // a Cmd of 33 bytes (cmd_cap 32), or one outside its pool: the marker
  // {type, ~0u, 1, 0}; the Cmd is not read (a null source)
  en.cmd_len = 33;
  CHECK(!prop_pack(v, en, (const uint8_t *)nullptr, true, pm));
  CHECK(eq4(pm[2], DRB_ENTRY_ENCODED, ~0u, 1, 0));
  CHECK(eq4(pm[0], 0, 0, 9, 0));
  en.cmd_len = 4;
  CHECK(!prop_pack(v, en, (const uint8_t *)nullptr, false, pm));
  CHECK(eq4(pm[2], DRB_ENTRY_ENCODED, ~0u, 1, 0));
}

int main() {
  open_cases();
  position_cases();
  propose_cases();
  replicate_cases();
  term_cases();
  tag_cases();
  row_cases();
  printf("ok %llu\n", g_checked);
  return 0;
}
