// The stand-alone program of tests/test_tanread_host.py: drb_tanread.hpp on
// the CPU, built with -fsanitize=address,undefined.
//
//   tanread_host_main COMMANDS
// COMMANDS holds one command per line; a log file is its bytes in hex ("-"
// when empty) and lives in a heap buffer of exactly its length, so that the
// sanitizer sees any read outside it.  One line of output per command:
//   scan FILE
//     <outcome> <valid_end> <n> {off:end:shard:replica:has_state:term:vote:
//     commit:first:last:n_entries}*     (what drb_tan_scan reports)
//   dump FILE
//     <outcome> <n> {off:payload hex:entries}*, entries "-" or a comma list
//     of term/index/type/key/client/series/responded/cmd hex
//   replica SHARD REPLICA BASE CMD_CAP W SNAPPY FILE...
//     pass 1 (tr_validate) and, for a good plan, pass 2 (tr_replay) into a
//     map: "<status> <files> <offset> <records> <entries> <term> <vote>
//     <commit> <last> <applied>|index/term/cmd hex,...|applied indexes"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../dragonboat_amd/csrc/drb_tanread.hpp"

using namespace drb;
typedef TanFile<TanFlatIn> File;

static int hexval(int c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

static std::string hex(const std::vector<uint8_t> &b) {
  if (b.empty()) return "-";
  std::string s;
  char t[3];
  for (uint8_t x : b) {
    snprintf(t, sizeof t, "%02x", x);
    s += t;
  }
  return s;
}

struct Buf {
  std::unique_ptr<uint8_t[]> p;  // exactly n bytes
  size_t n = 0;
  File file() const { return File{TanFlatIn{p.get()}, 0, n}; }
};

static Buf parse(const std::string &tok) {
  Buf b;
  if (tok == "-") {
    b.p.reset(new uint8_t[0]);
    return b;
  }
  b.n = tok.size() / 2;
  b.p.reset(new uint8_t[b.n]);
  for (size_t i = 0; i < b.n; ++i)
    b.p[i] = (uint8_t)(hexval(tok[2 * i]) * 16 + hexval(tok[2 * i + 1]));
  return b;
}

// keeps every Cmd
struct KeepCmd {
  std::vector<uint8_t> bytes;
  template <class C>
  void cmd(C &c, const TrEntry &e) {
    bytes.clear();
    for (uint32_t i = 0; i < e.cmd_len; ++i) bytes.push_back((uint8_t)c.byte());
  }
};

static void do_scan(const Buf &b) {
  const File f = b.file();
  TanWalk w;
  std::string recs;
  uint64_t valid_end = 0, n = 0;
  int oc;
  for (;;) {
    TrScanRec r;
    oc = tr_scan_record(f, w, r);
    if (oc != TR_REC) break;
    char t[400];
    snprintf(t, sizeof t, " %llu:%llu:%llu:%llu:%u:%llu:%llu:%llu:%llu:%llu:%u",
             (unsigned long long)r.offset, (unsigned long long)r.end,
             (unsigned long long)r.shard_id, (unsigned long long)r.replica_id,
             r.has_state, (unsigned long long)r.term,
             (unsigned long long)r.vote, (unsigned long long)r.commit,
             (unsigned long long)r.first_index,
             (unsigned long long)r.last_index, r.n_entries);
    recs += t;
    valid_end = r.end;
    n++;
  }
  printf("%d %llu %llu%s\n", oc, (unsigned long long)valid_end,
         (unsigned long long)n, recs.c_str());
}

static void do_dump(const Buf &b) {
  const File f = b.file();
  TanWalk w;
  std::string recs;
  uint64_t n = 0;
  int oc;
  for (;;) {
    const TanWalk before = w;
    const uint64_t off = tr_offset(w);
    uint64_t rlen;
    oc = tr_walk_record(f, w, true, &rlen);
    if (oc != TR_REC) break;
    std::vector<uint8_t> payload;
    {
      TanCur<File> c(f, before, rlen);
      while (c.left) payload.push_back((uint8_t)c.byte());
      if (c.bad) oc = TR_MALFORMED;
    }
    TanCur<File> c(f, before, rlen);
    TrUpdate u;
    std::string ents;
    bool ok = tr_update_head(c, u);
    for (uint32_t k = 0; ok && k < u.n_entries; ++k) {
      uint32_t len;
      TrEntry e;
      KeepCmd sink;
      ok = tr_entry_len(c, &len) && tr_entry(c, len, e, sink);
      if (!ok) break;
      if (e.cmd_len == 0) sink.bytes.clear();
      char t[300];
      snprintf(t, sizeof t, "%s%llu/%llu/%u/%llu/%llu/%llu/%llu/",
               k ? "," : "", (unsigned long long)e.term,
               (unsigned long long)e.index, e.type, (unsigned long long)e.key,
               (unsigned long long)e.client_id,
               (unsigned long long)e.series_id,
               (unsigned long long)e.responded_to);
      ents += t + hex(sink.bytes);
    }
    bool snap = false;
    ok = ok && tr_update_tail(c, &snap);
    if (!ok) {
      oc = TR_MALFORMED;
      break;
    }
    recs += " " + std::to_string(off) + ":" + hex(payload) + ":" +
            (ents.empty() ? "-" : ents);
    n++;
  }
  printf("%d %llu%s\n", oc, (unsigned long long)n, recs.c_str());
}

// pass 2 into a map: the log as the overwrite rule leaves it.  `ring` is the
// device's window: slot index mod W holds the last index placed there, and
// an apply of an entry that is no longer its slot's occupant fails (the
// device would apply another entry's Cmd) -- pass 1 must have refused the log
struct MapPlacer {
  uint64_t base;
  std::vector<uint64_t> ring;
  std::map<uint64_t, std::pair<uint64_t, std::vector<uint8_t>>> log;
  std::vector<uint8_t> pending;
  std::vector<uint64_t> applied;
  std::vector<uint64_t> applied_terms;
  template <class C>
  void cmd(C &c, const TrEntry &e) {
    pending.clear();
    for (uint32_t i = 0; i < e.cmd_len; ++i)
      pending.push_back((uint8_t)c.byte());
  }
  void place(const TrEntry &e) {
    if (e.cmd_len == 0) pending.clear();
    // "new writes always overwrite old entries": what follows goes too
    log.erase(log.lower_bound(e.index), log.end());
    log[e.index] = {e.term, pending};
    pending.clear();
    ring[e.index % ring.size()] = e.index;
  }
  bool apply(uint64_t index) {
    if (!log.count(index) || ring[index % ring.size()] != index) return false;
    applied.push_back(index);
    applied_terms.push_back(log[index].first);
    return true;
  }
};

static void do_replica(const std::vector<std::string> &tok) {
  TrLimits lim;
  lim.shard_id = strtoull(tok[1].c_str(), nullptr, 10);
  lim.replica_id = strtoull(tok[2].c_str(), nullptr, 10);
  lim.base_index = strtoull(tok[3].c_str(), nullptr, 10);
  lim.cmd_cap = (uint32_t)strtoul(tok[4].c_str(), nullptr, 10);
  lim.W = (uint32_t)strtoul(tok[5].c_str(), nullptr, 10);
  lim.snappy = (uint32_t)strtoul(tok[6].c_str(), nullptr, 10);
  std::vector<Buf> bufs;
  std::vector<File> files;
  for (size_t i = 7; i < tok.size(); ++i) bufs.push_back(parse(tok[i]));
  for (const Buf &b : bufs) files.push_back(b.file());
  const TrPlan pl = tr_validate(files, (uint32_t)files.size(), lim);
  MapPlacer mp;
  mp.base = lim.base_index;
  mp.ring.assign(lim.W ? lim.W : 1, 0);
  uint64_t applied = 0;
  uint32_t status = pl.status;
  if (status == TRS_OK || status == TRS_TAIL_CUT)
    if (!tr_replay(files, pl, lim, mp, &applied))
      status = TRS_APPLY_STOPPED;
  // the window pass 2 leaves: [ring_lo, last] must all be their slots'
  // occupants (drb_recover.hpp computes ring_lo the same way)
  if (status == TRS_OK || status == TRS_TAIL_CUT) {
    const uint64_t high = pl.high_index > pl.last_index ? pl.high_index
                                                        : pl.last_index;
    uint64_t lo = high + 1 > lim.W ? high + 1 - lim.W : 1;
    if (lo > pl.last_index) lo = pl.last_index ? pl.last_index : 1;
    if (lo <= lim.base_index) lo = lim.base_index + 1;
    for (uint64_t i = lo; i <= pl.last_index; ++i)
      if (mp.ring[i % mp.ring.size()] != i) status = 100;  // stale window
  }
  printf("%u %u %llu %llu %llu %llu %llu %llu %llu %llu|", status, pl.files,
         (unsigned long long)pl.offset, (unsigned long long)pl.records,
         (unsigned long long)pl.entries, (unsigned long long)pl.term,
         (unsigned long long)pl.vote, (unsigned long long)pl.commit,
         (unsigned long long)pl.last_index, (unsigned long long)applied);
  bool first = true;
  for (const auto &kv : mp.log) {
    printf("%s%llu/%llu/%s", first ? "" : ",", (unsigned long long)kv.first,
           (unsigned long long)kv.second.first, hex(kv.second.second).c_str());
    first = false;
  }
  printf("|");
  for (size_t i = 0; i < mp.applied.size(); ++i)
    printf("%s%llu/%llu", i ? "," : "", (unsigned long long)mp.applied[i],
           (unsigned long long)mp.applied_terms[i]);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  std::string line;
  int ch;
  for (;;) {
    line.clear();
    while ((ch = fgetc(f)) != EOF && ch != '\n') line += (char)ch;
    if (line.empty() && ch == EOF) break;
    std::vector<std::string> tok;
    size_t i = 0;
    while (i < line.size()) {
      size_t j = line.find(' ', i);
      if (j == std::string::npos) j = line.size();
      if (j > i) tok.push_back(line.substr(i, j - i));
      i = j + 1;
    }
    if (tok.empty()) continue;
    if (tok[0] == "scan" && tok.size() == 2) do_scan(parse(tok[1]));
    else if (tok[0] == "dump" && tok.size() == 2) do_dump(parse(tok[1]));
    else if (tok[0] == "replica" && tok.size() >= 7) do_replica(tok);
    else return 3;
    if (ch == EOF) break;
  }
  fclose(f);
  return 0;
}
