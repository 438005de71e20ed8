// CPU driver for the per-message wire decoder (drb_msgdec.hpp), built by
// tests/test_msgdecode_host.py with -fsanitize=address,undefined.  Reads a
// file of length-prefixed messages (u32 little endian, then the bytes) and a
// cmd_cap, and prints what the decoder made of each, both passes:
//   msg <k> <count outcome> <count n_ent> <decode outcome> <decode n_ent>
//       <type> <to> <from> <shard> <term> <log_term> <log_index> <commit>
//       <reject> <hint> <hint_high>
//   ent <term> <index> <type> <key> <client_id> <series_id> <responded_to>
//       <cmd_off> <cmd_len>                    (n_ent lines, decode pass)
// outcome: 0 ok, 1 bad, 2 snapshot, 3 big (a Cmd over cmd_cap).  Every
// message sits in a heap allocation of exactly its size, so a read past
// either end is an AddressSanitizer report.  Test infrastructure only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../dragonboat_amd/csrc/drb_msgdec.hpp"

static uint32_t outcome(uint32_t r, bool big) {
  return r == drb::ING_OK && big ? drb::ING_BIG : r;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) return 2;
  const uint32_t cmd_cap = (uint32_t)strtoul(argv[2], nullptr, 10);
  std::vector<drb_entry> ents;
  for (unsigned long k = 0;; ++k) {
    uint8_t lb[4];
    const size_t got = fread(lb, 1, 4, fp);
    if (got == 0) break;
    if (got != 4) return 3;
    const uint32_t n = lb[0] | lb[1] << 8 | lb[2] << 16 | (uint32_t)lb[3] << 24;
    // (malloc(0) may return NULL: one byte then, outside the message)
    uint8_t *msg = (uint8_t *)malloc(n ? n : 1);
    if (!msg || (n && fread(msg, 1, n, fp) != n)) return 3;
    const uint8_t *in = msg;
    if (n == 0) in = msg + 1;  // no byte of an empty message is readable
    drb::DecMsg m1, m2;
    bool big1 = false, big2 = false;
    uint32_t r1 = drb::d_message(in, n, m1, nullptr, 0, cmd_cap, big1);
    r1 = outcome(r1, big1);
    // the decode pass writes n_ent entries: an array of exactly the count
    // pass's size, as k_ing_decode's share of the entry buffer is (a
    // refused message's: the entries before the refusal)
    const uint32_t cnt = m1.n_ent;
    drb_entry *e = (drb_entry *)malloc(sizeof(drb_entry) * (cnt ? cnt : 1));
    if (!e) return 3;
    uint32_t r2 = drb::d_message(in, n, m2, e, 0, cmd_cap, big2);
    r2 = outcome(r2, big2);
    printf("msg %lu %u %u %u %u %u %llu %llu %llu %llu %llu %llu %llu %u "
           "%llu %llu\n",
           k, r1, m1.n_ent, r2, m2.n_ent, m2.type, (unsigned long long)m2.to,
           (unsigned long long)m2.from, (unsigned long long)m2.shard,
           (unsigned long long)m2.term, (unsigned long long)m2.log_term,
           (unsigned long long)m2.log_index, (unsigned long long)m2.commit,
           m2.reject, (unsigned long long)m2.hint,
           (unsigned long long)m2.hint_high);
    if (r2 != drb::ING_BAD)
      for (uint32_t x = 0; x < m2.n_ent; ++x)
        printf("ent %llu %llu %u %llu %llu %llu %llu %llu %u\n",
               (unsigned long long)e[x].term, (unsigned long long)e[x].index,
               e[x].type, (unsigned long long)e[x].key,
               (unsigned long long)e[x].client_id,
               (unsigned long long)e[x].series_id,
               (unsigned long long)e[x].responded_to,
               (unsigned long long)e[x].cmd_off, e[x].cmd_len);
    free(e);
    free(msg);
  }
  fclose(fp);
  return 0;
}
