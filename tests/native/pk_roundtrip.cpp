// pk_roundtrip.cpp -- the packed 64 B replica record's codec
// (drb_layout.hpp pk_encode / pk_decode) at every field's range boundary.
//
// For each combination of boundary values the program encodes a record,
// checks every field's 16-bit (8-bit for ids) code against the expectation
// stated in the tables below -- in range with that code, or the escape
// code with the value in the overflow array -- and checks that decoding
// returns the values.  The overflow array is filled with junk first: an
// in-range field must leave its slot alone on encode and must not read it
// on decode.  The expectations are literal tables, not calls of the
// pk_*_code helpers, so an off-by-one made the same way in encode and
// decode still fails.
//
// Built by tests/test_packed_record.py with -fsanitize=address,undefined.
// Prints "ok <combinations>" and exits 0, or the first mismatch and 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../dragonboat_amd/csrc/drb_layout.hpp"

using namespace drb;

static unsigned long long g_checked = 0;

[[noreturn]] static void fail(const char *what, int field, uint64_t got,
                              uint64_t want, uint64_t last, uint64_t term) {
  printf("FAIL %s field %d got %llx want %llx (last %llx term %llx)\n", what,
         field, (unsigned long long)got, (unsigned long long)want,
         (unsigned long long)last, (unsigned long long)term);
  exit(1);
}

// ---- the expectations ---------------------------------------------------
struct IdxCase {
  int64_t d;       // value = last + d
  bool esc;        // an ordinary index field escapes
  bool guard_esc;  // the ring guard escapes (0x7fff is its +inf)
};
static const IdxCase IDX[] = {
    {-40000, true, true},   {-32769, true, true},  {-32768, true, true},
    {-32767, false, false}, {-1, false, false},    {0, false, false},
    {1, false, false},      {32766, false, false}, {32767, false, true},
    {32768, true, true},
};
constexpr int N_IDX = sizeof(IDX) / sizeof(IDX[0]);
static const uint64_t LASTS[] = {4, 32767, 32768, 1ull << 32,
                                 (1ull << 63) + 7};

struct TermCase {
  uint64_t dist;  // value = term - dist (wrapping: then value > term)
  bool esc;       // when value <= term
};
static const TermCase TERMD[] = {
    {0, false},    {1, false},    {65534, false},
    {65535, true}, {65536, true}, {~0ull /* value = term + 1 */, true},
};
constexpr int N_TERMD = sizeof(TERMD) / sizeof(TERMD[0]);
static const uint64_t TERMS[] = {2, 65536, 65537, 1ull << 49, ~0ull - 1};

struct U16Case {
  uint64_t v;
  bool esc;
};
static const U16Case TICKS[] = {{65534, false}, {65535, true}, {65536, true}};
static const U16Case IDS[] = {{254, false}, {255, true}, {256, true}};

static uint64_t junk(int f) { return 0xDEAD0000BEEF0000ull + (uint64_t)f; }

// One record: idx[i] selects IDX[] for PIdx field i (-1: the guard's ~0),
// tc / kc / dc rotate the term, tick and id cases over their three fields.
static void one(uint64_t last, uint64_t term, const int *idx, int tc, int kc,
                int dc) {
  uint64_t vals[NUM_U64], over[NUM_U64], back[NUM_U64];
  uint32_t w[16];
  bool esc[NUM_U64] = {};
  uint32_t code[NUM_U64] = {};
  for (int f = 0; f < NUM_U64; ++f) {
    vals[f] = 0;
    over[f] = junk(f);
    back[f] = 0x5151515151515151ull;
  }
  vals[F_LAST_INDEX] = last;
  vals[F_TERM] = term;
  for (int i = 0; i < NUM_PI; ++i) {
    const int f = pi_field(i);
    const bool guard = i == PI_RING_GUARD;
    if (idx[i] < 0) {  // PK_INF16
      vals[f] = ~0ull;
      esc[f] = false;
      code[f] = 0x7fffu;
      continue;
    }
    const IdxCase &c = IDX[idx[i]];
    vals[f] = last + (uint64_t)c.d;
    esc[f] = guard ? c.guard_esc : c.esc;
    code[f] = esc[f] ? 0x8000u : ((uint32_t)(int32_t)c.d & 0xffffu);
    if (guard && vals[f] == ~0ull) {  // last + d wrapped onto +inf
      esc[f] = false;
      code[f] = 0x7fffu;
    }
  }
  const int tf[3] = {F_APPLIED_TO_TERM, F_PREV_TERM, F_SM_TERM};
  for (int k = 0; k < 3; ++k) {
    const TermCase &c = TERMD[(tc + k) % N_TERMD];
    const uint64_t x = term - c.dist;
    vals[tf[k]] = x;
    esc[tf[k]] = x > term ? true : c.esc;
    code[tf[k]] = esc[tf[k]] ? 0xffffu : (uint32_t)c.dist;
  }
  const int uf[3] = {F_ELECTION_TICK, F_HEARTBEAT_TICK, F_RAND_TIMEOUT};
  for (int k = 0; k < 3; ++k) {
    const U16Case &c = TICKS[(kc + k) % 3];
    vals[uf[k]] = c.v;
    esc[uf[k]] = c.esc;
    code[uf[k]] = c.esc ? 0xffffu : (uint32_t)c.v;
  }
  const int df[3] = {F_VOTE, F_LEADER_ID, F_PREV_VOTE};
  for (int k = 0; k < 3; ++k) {
    const U16Case &c = IDS[(dc + k) % 3];
    vals[df[k]] = c.v;
    esc[df[k]] = c.esc;
    code[df[k]] = c.esc ? 0xffu : (uint32_t)c.v;
  }
  // the fields that only ever live in the u64 array
  const int plain[] = {F_TICK_COUNT, F_KV_COUNT, F_QS_TICK, F_QS_IDLE,
                       F_QS_SINCE,   F_QS_EXIT,  F_RNG,     F_QS_BASE};
  bool is_plain[NUM_U64] = {};
  for (int f : plain) {
    vals[f] = 0x0123456789abcdefull * (uint64_t)(f + 1);
    over[f] = vals[f];
    is_plain[f] = true;
  }

  pk_encode(w, vals, over);

  // the codes, as stored
  if (w[0] != (uint32_t)last || w[1] != (uint32_t)(last >> 32))
    fail("last words", F_LAST_INDEX, w[0], last, last, term);
  if (w[2] != (uint32_t)term || w[3] != (uint32_t)(term >> 32))
    fail("term words", F_TERM, w[2], term, last, term);
  for (int i = 0; i < NUM_PI; ++i) {
    const uint32_t got = (w[4 + i / 2] >> (16 * (i & 1))) & 0xffffu;
    if (got != code[pi_field(i)])
      fail("index code", pi_field(i), got, code[pi_field(i)], last, term);
  }
  const uint32_t tgot[3] = {w[11] & 0xffffu, w[11] >> 16, w[12] & 0xffffu};
  for (int k = 0; k < 3; ++k)
    if (tgot[k] != code[tf[k]])
      fail("term code", tf[k], tgot[k], code[tf[k]], last, term);
  const uint32_t ugot[3] = {w[12] >> 16, w[13] & 0xffffu, w[13] >> 16};
  for (int k = 0; k < 3; ++k)
    if (ugot[k] != code[uf[k]])
      fail("tick code", uf[k], ugot[k], code[uf[k]], last, term);
  for (int k = 0; k < 3; ++k)
    if (((w[14] >> (8 * k)) & 0xffu) != code[df[k]])
      fail("id code", df[k], (w[14] >> (8 * k)) & 0xffu, code[df[k]], last,
           term);
  if ((w[14] >> 24) != 0 || w[15] != 0)
    fail("spare bits", -1, w[15], 0, last, term);

  // the overflow array: the value where the field escaped, junk elsewhere
  for (int f = 0; f < NUM_U64; ++f) {
    if (f == F_LAST_INDEX || f == F_TERM || is_plain[f]) continue;
    const uint64_t want = esc[f] ? vals[f] : junk(f);
    if (over[f] != want) fail("overflow slot", f, over[f], want, last, term);
    if (!esc[f] && vals[f] == junk(f)) fail("junk collides", f, 0, 0, 0, 0);
  }
  if (over[F_LAST_INDEX] != junk(F_LAST_INDEX) ||
      over[F_TERM] != junk(F_TERM))
    fail("overflow slot of last/term", F_TERM, 0, 0, last, term);

  pk_decode(w, over, back);
  for (int f = 0; f < NUM_U64; ++f) {
    if (f == F_SAVE_BASE) continue;  // not part of the record
    if (back[f] != vals[f]) fail("decode", f, back[f], vals[f], last, term);
  }
  ++g_checked;
}

int main() {
  // index configurations: every field singly over IDX (the others at 0),
  // the guard's +inf against its neighbours, and all fields together
  static int cfg[NUM_PI * N_IDX + N_IDX * N_IDX + 8][NUM_PI];
  int n_cfg = 0;
  const int zero = 5;  // IDX[5].d == 0
  if (IDX[zero].d != 0) return 2;
  for (int i = 0; i < NUM_PI; ++i)
    for (int c = 0; c < N_IDX; ++c) {
      for (int j = 0; j < NUM_PI; ++j) cfg[n_cfg][j] = zero;
      cfg[n_cfg++][i] = c;
    }
  // ring guard ~0 while every ordinary field sits at 32766 / 32767, and
  // the guard at 32766 / 32767 itself
  for (int c = 7; c <= 8; ++c) {
    for (int j = 0; j < NUM_PI; ++j) cfg[n_cfg][j] = c;
    cfg[n_cfg++][PI_RING_GUARD] = -1;
    for (int j = 0; j < NUM_PI; ++j) cfg[n_cfg][j] = zero;
    cfg[n_cfg++][PI_RING_GUARD] = -1;
  }
  // all together: field i at IDX[(c + s * i) % N_IDX], so neighbours in a
  // word carry every pair of cases
  for (int c = 0; c < N_IDX; ++c)
    for (int s = 0; s < N_IDX; ++s) {
      for (int j = 0; j < NUM_PI; ++j) cfg[n_cfg][j] = (c + s * j) % N_IDX;
      ++n_cfg;
    }

  for (uint64_t last : LASTS)
    for (uint64_t term : TERMS)
      for (int q = 0; q < n_cfg; ++q)
        for (int tc = 0; tc < N_TERMD; ++tc)
          for (int kc = 0; kc < 3; ++kc)
            for (int dc = 0; dc < 3; ++dc) one(last, term, cfg[q], tc, kc, dc);
  printf("ok %llu\n", g_checked);
  return 0;
}
