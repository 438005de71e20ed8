// pk_counters.cpp -- tick_count and kv_count of the packed replica record
// (drb_layout.hpp): the u64 field plus a 16-bit delta in word 15, low half
// ticks, high half KV updates.
//
// Checks, over field values 0, 1, 2^32, 2^63 and deltas 0, 1, 0xfffe, 0xffff
// in either half (every pair of them),
//   - that pk_decode returns field + delta for both counters,
//   - that neither half's delta leaks into the other counter and that every
//     other field decodes to what a zero word 15 decodes to,
//   - that pk_encode writes word 15 = 0 and pk_decode of its record with the
//     counters' values in the u64 array is the identity,
//   - pk_count_add: the delta holds sums up to 0xffff, a sum past it comes
//     back whole with the delta zeroed, the other half untouched, and
//     field + delta is what was counted either way.
//
// Built by tests/test_packed_counters.py with -fsanitize=address,undefined.
// Prints "ok <checks>" and exits 0, or the first mismatch and 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../dragonboat_amd/csrc/drb_layout.hpp"

using namespace drb;

static unsigned long long g_checked = 0;

[[noreturn]] static void fail(const char *what, int field, uint64_t got,
                              uint64_t want) {
  printf("FAIL %s field %d got %llx want %llx\n", what, field,
         (unsigned long long)got, (unsigned long long)want);
  exit(1);
}

static const uint64_t FIELDS[] = {0, 1, 1ull << 32, 1ull << 63};
static const uint32_t DELTAS[] = {0, 1, 0xfffeu, 0xffffu};

// a record with every field in range and distinct, and its u64 array
static void base_record(uint64_t *vals, uint64_t *over, uint32_t *w) {
  for (int f = 0; f < NUM_U64; ++f) vals[f] = over[f] = 0;
  vals[F_LAST_INDEX] = 1000;
  vals[F_TERM] = 7;
  for (int i = 0; i < NUM_PI; ++i) vals[pi_field(i)] = 1000 - 3 * (i + 1);
  vals[F_RING_GUARD] = ~0ull;
  vals[F_APPLIED_TO_TERM] = 6;
  vals[F_PREV_TERM] = 7;
  vals[F_SM_TERM] = 5;
  vals[F_ELECTION_TICK] = 3;
  vals[F_HEARTBEAT_TICK] = 1;
  vals[F_RAND_TIMEOUT] = 17;
  vals[F_VOTE] = 2;
  vals[F_LEADER_ID] = 2;
  vals[F_PREV_VOTE] = 2;
  const int plain[] = {F_QS_TICK, F_QS_IDLE, F_QS_SINCE, F_QS_EXIT, F_RNG,
                       F_QS_BASE};
  for (int f : plain) vals[f] = over[f] = 0x1111111111111111ull * (f + 1);
  pk_encode(w, vals, over);
}

static void decode_cases() {
  for (uint64_t tf : FIELDS)
    for (uint64_t kf : FIELDS)
      for (uint32_t td : DELTAS)
        for (uint32_t kd : DELTAS) {
          uint64_t vals[NUM_U64], over[NUM_U64], ref[NUM_U64], back[NUM_U64];
          uint32_t w[16];
          base_record(vals, over, w);
          if (w[15] != 0) fail("encode word 15", -1, w[15], 0);
          over[F_TICK_COUNT] = tf;
          over[F_KV_COUNT] = kf;
          for (int f = 0; f < NUM_U64; ++f) ref[f] = back[f] = 0;
          pk_decode(w, over, ref);  // deltas zero
          if (ref[F_TICK_COUNT] != tf)
            fail("zero delta", F_TICK_COUNT, ref[F_TICK_COUNT], tf);
          if (ref[F_KV_COUNT] != kf)
            fail("zero delta", F_KV_COUNT, ref[F_KV_COUNT], kf);
          uint32_t w2[16];
          for (int q = 0; q < 16; ++q) w2[q] = w[q];
          w2[15] = td | (kd << 16);
          pk_decode(w2, over, back);
          if (back[F_TICK_COUNT] != tf + td)
            fail("tick_count", F_TICK_COUNT, back[F_TICK_COUNT], tf + td);
          if (back[F_KV_COUNT] != kf + kd)
            fail("kv_count", F_KV_COUNT, back[F_KV_COUNT], kf + kd);
          for (int f = 0; f < NUM_U64; ++f) {
            if (f == F_TICK_COUNT || f == F_KV_COUNT) continue;
            if (back[f] != ref[f]) fail("other field", f, back[f], ref[f]);
          }
          // the decode left the record and the array alone
          if (w2[15] != (td | (kd << 16))) fail("word 15", -1, w2[15], td);
          if (over[F_TICK_COUNT] != tf || over[F_KV_COUNT] != kf)
            fail("u64 array", F_TICK_COUNT, over[F_TICK_COUNT], tf);
          ++g_checked;
        }
}

// pk_encode then pk_decode: the identity with word 15 = 0, the counters
// whole in their fields
static void roundtrip_cases() {
  for (uint64_t tv : FIELDS)
    for (uint64_t kv : FIELDS)
      for (uint32_t td : DELTAS)
        for (uint32_t kd : DELTAS) {
          uint64_t vals[NUM_U64], over[NUM_U64], back[NUM_U64];
          uint32_t w[16];
          base_record(vals, over, w);
          vals[F_TICK_COUNT] = tv + td;  // (what a decode with deltas gave)
          vals[F_KV_COUNT] = kv + kd;
          for (int q = 0; q < 16; ++q) w[q] = 0xa5a5a5a5u;
          pk_encode(w, vals, over);
          if (w[15] != 0) fail("encode word 15", -1, w[15], 0);
          // the callers store the counters' values into the array
          over[F_TICK_COUNT] = vals[F_TICK_COUNT];
          over[F_KV_COUNT] = vals[F_KV_COUNT];
          for (int f = 0; f < NUM_U64; ++f) back[f] = 0x5151515151515151ull;
          pk_decode(w, over, back);
          for (int f = 0; f < NUM_U64; ++f) {
            if (f == F_SAVE_BASE) continue;  // not part of the record
            if (back[f] != vals[f]) fail("roundtrip", f, back[f], vals[f]);
          }
          ++g_checked;
        }
}

static void count_add_cases() {
  const uint32_t ADDS[] = {1, 2, 0xffffu, 0x10000u, 1000000u};
  for (int hi = 0; hi < 2; ++hi)
    for (uint32_t d0 : DELTAS)
      for (uint32_t other : DELTAS)
        for (uint32_t n : ADDS) {
          uint32_t w[16];
          for (int q = 0; q < 16; ++q) w[q] = 0x01010101u * (uint32_t)(q + 1);
          uint32_t keep[16];
          w[15] = hi ? (other | (d0 << 16)) : (d0 | (other << 16));
          for (int q = 0; q < 16; ++q) keep[q] = w[q];
          const uint32_t fold = pk_count_add(w, hi, n);
          const uint32_t mine = (w[15] >> (16 * hi)) & 0xffffu;
          const uint32_t theirs = (w[15] >> (16 * (1 - hi))) & 0xffffu;
          const uint64_t sum = (uint64_t)d0 + n;
          if (theirs != other) fail("other half", hi, theirs, other);
          for (int q = 0; q < 15; ++q)
            if (w[q] != keep[q]) fail("other word", q, w[q], keep[q]);
          if (sum <= 0xffffu) {
            if (fold != 0 || mine != sum) fail("held", hi, mine, sum);
          } else {
            if (fold != sum || mine != 0) fail("fold", hi, fold, sum);
          }
          if ((uint64_t)fold + mine != sum) fail("sum", hi, fold + mine, sum);
          ++g_checked;
        }
  // 70,000 single counts from zero cross 0xffff once
  uint32_t w[16] = {0};
  uint64_t field = 0;
  for (int i = 0; i < 70000; ++i) field += pk_count_add(w, PK_CNT_TICK, 1);
  if (field != 0x10000u || (w[15] & 0xffffu) != 70000 - 0x10000 ||
      (w[15] >> 16) != 0)
    fail("70000 ticks", F_TICK_COUNT, field + (w[15] & 0xffffu), 70000);
  ++g_checked;
}

int main() {
  decode_cases();
  roundtrip_cases();
  count_add_cases();
  printf("ok %llu\n", g_checked);
  return 0;
}
