// The stand-alone program of tests/test_tanmux_host.py: drb_tanmux.hpp on the
// CPU, built with -fsanitize=address,undefined.  Files travel as in
// tanread_host_main.cc (hex, a heap buffer of exactly the file's length);
// that program's commands (scan, dump, replica) and its placer are taken from
// its source, so both read paths run in one process under one placer.
//
//   index FILE
//     the block index of one file, the blocks summarized in REVERSE order (a
//     block's summary needs nothing from the blocks before it), composed, its
//     records listed: "<outcome> <valid_end> <n> {off:end:shard:replica}*"
//     (off / end as drb_tan_scan reports them; outcome 5 when a record's ids
//     do not parse, the list ending in front of it)
//   seq FILE
//     the same line from the sequential reader (tr_scan_record)
//   mux SLOT FIRST_SHARD GROUPS BASE CMD_CAP W SNAPPY {KEY NFILES FILE...}*
//     the logs (SLOT, KEY) through index, composition, record list, partition
//     and the per-replica passes:
//     "key,status,log,offset,records ...@g~<replica line>;..." for every
//     group of the given keys, <replica line> as the replica command prints
#define main tanread_host_main
#include "tanread_host_main.cc"
#undef main

#include <algorithm>

#include "../dragonboat_amd/csrc/drb_tanmux.hpp"

static void print_index_line(int oc, uint64_t vend, const std::string &recs,
                             uint64_t n) {
  printf("%d %llu %llu%s\n", oc, (unsigned long long)vend,
         (unsigned long long)n, recs.c_str());
}

struct Headers {
  std::vector<uint64_t> at;
  void operator()(uint32_t, uint64_t hdr) { at.push_back(hdr); }
};

static void do_index(const Buf &b) {
  const File f = b.file();
  const uint64_t nb = tm_blocks(f.size);
  std::vector<TmBlock> sum(nb);
  for (uint64_t k = nb; k-- > 0;) sum[k] = tm_summarize(f, k);
  std::vector<uint8_t> entry(nb + 1);
  std::vector<uint32_t> cnt(nb + 1);
  const TmFileOut o = tm_compose(sum.data(), nb, f.size, entry.data(),
                                 cnt.data());
  std::string recs;
  uint64_t n = 0, prev_end = 0;
  int oc = (int)o.outcome;
  for (uint64_t k = 0; k < nb && oc != TR_MALFORMED; ++k) {
    Headers h;
    tm_block_records(f, k, entry[k], cnt[k], h);
    if (h.at.size() != cnt[k]) exit(4);
    for (uint64_t hdr : h.at) {
      uint64_t rlen, end, shard, replica;
      if (tm_record(f, hdr, &rlen, &end, &shard, &replica) != TRS_OK) {
        oc = TR_MALFORMED;
        break;
      }
      char t[200];
      snprintf(t, sizeof t, " %llu:%llu:%llu:%llu",
               (unsigned long long)prev_end, (unsigned long long)end,
               (unsigned long long)shard, (unsigned long long)replica);
      recs += t;
      prev_end = end;
      n++;
    }
  }
  if (oc != TR_MALFORMED && (n != o.records || prev_end != o.valid_end))
    exit(5);
  print_index_line(oc, prev_end, recs, n);
}

static void do_seq(const Buf &b) {
  const File f = b.file();
  TanWalk w;
  std::string recs;
  uint64_t vend = 0, n = 0;
  int oc;
  for (;;) {
    TrScanRec r;
    oc = tr_scan_record(f, w, r);
    if (oc != TR_REC) break;
    char t[200];
    snprintf(t, sizeof t, " %llu:%llu:%llu:%llu", (unsigned long long)r.offset,
             (unsigned long long)r.end, (unsigned long long)r.shard_id,
             (unsigned long long)r.replica_id);
    recs += t;
    vend = r.end;
    n++;
  }
  print_index_line(oc, vend, recs, n);
}

static void do_mux(const std::vector<std::string> &tok) {
  const uint32_t slot = (uint32_t)strtoul(tok[1].c_str(), nullptr, 10);
  const uint64_t first_shard = strtoull(tok[2].c_str(), nullptr, 10);
  const uint64_t groups = strtoull(tok[3].c_str(), nullptr, 10);
  TrLimits lim;
  lim.replica_id = slot + 1;
  lim.base_index = strtoull(tok[4].c_str(), nullptr, 10);
  lim.cmd_cap = (uint32_t)strtoul(tok[5].c_str(), nullptr, 10);
  lim.W = (uint32_t)strtoul(tok[6].c_str(), nullptr, 10);
  lim.snappy = (uint32_t)strtoul(tok[7].c_str(), nullptr, 10);
  // the logs: each file a buffer of its own; TmFile.off is unused here (a
  // record's file is looked up in `bufs`)
  struct Log {
    uint32_t key, f0, nf;
  };
  std::vector<Log> logs;
  std::vector<Buf> bufs;
  std::vector<TmFile> files;
  uint32_t nblk = 0;
  for (size_t i = 8; i < tok.size();) {
    Log lg;
    lg.key = (uint32_t)strtoul(tok[i].c_str(), nullptr, 10);
    lg.nf = (uint32_t)strtoul(tok[i + 1].c_str(), nullptr, 10);
    lg.f0 = (uint32_t)files.size();
    i += 2;
    for (uint32_t k = 0; k < lg.nf; ++k, ++i) {
      bufs.push_back(parse(tok[i]));
      files.push_back(TmFile{0, bufs.back().n, k, nblk});
      nblk += (uint32_t)tm_blocks(bufs.back().n);
    }
    logs.push_back(lg);
  }
  // pass A, every block of every file, last block first
  std::vector<TmBlock> sum(nblk + 1);
  for (size_t fi = files.size(); fi-- > 0;)
    for (uint64_t k = tm_blocks(files[fi].len); k-- > 0;)
      sum[files[fi].blk0 + k] = tm_summarize(bufs[fi].file(), k);
  std::vector<uint8_t> entry(nblk + 1);
  std::vector<uint32_t> cnt(nblk + 1);
  std::vector<TmLogOut> lout;
  for (const Log &lg : logs)
    lout.push_back(tm_compose_log(files.data() + lg.f0, lg.nf, sum.data(),
                                  entry.data(), cnt.data(), nullptr));
  // pass B: the record table in (log, file, block) order, each record's
  // replica; the first record in log order that is not the log's refuses it
  struct Owned {
    TmRec rec;
    uint64_t q;  // the group; `groups`: none
  };
  std::vector<Owned> recs;
  for (size_t li = 0; li < logs.size(); ++li) {
    const Log &lg = logs[li];
    bool bad = false;
    for (uint32_t k = 0; k < lg.nf; ++k) {
      const uint32_t fi = lg.f0 + k;
      const File f = bufs[fi].file();
      for (uint64_t b = 0; b < tm_blocks(f.size); ++b) {
        Headers h;
        tm_block_records(f, b, entry[files[fi].blk0 + b],
                         cnt[files[fi].blk0 + b], h);
        if (h.at.size() != cnt[files[fi].blk0 + b]) exit(4);
        for (uint64_t hdr : h.at) {
          uint64_t rlen = 0, end, shard, replica, g = groups;
          uint32_t st = tm_record(f, hdr, &rlen, &end, &shard, &replica);
          if (st == TRS_OK)
            st = tm_owner_status(shard, replica, first_shard, groups, slot,
                                 lg.key, &g);
          if (st != TRS_OK && !bad && lout[li].status < TRS_CORRUPT) {
            lout[li].status = st;
            bad = true;
          }
          recs.push_back(Owned{TmRec{hdr, fi, (uint32_t)rlen},
                               st == TRS_OK ? g : groups});
        }
      }
    }
  }
  // the partition: a stable sort on the owner
  std::vector<uint32_t> order(recs.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return recs[a].q < recs[b].q;
  });
  std::string out;
  for (size_t li = 0; li < logs.size(); ++li) {
    char t[200];
    snprintf(t, sizeof t, "%s%u,%u,%u,%llu,%llu", li ? " " : "", logs[li].key,
             lout[li].status, lout[li].log,
             (unsigned long long)lout[li].offset,
             (unsigned long long)lout[li].records);
    out += t;
  }
  printf("%s@", out.c_str());
  // a replica's record list over the buffers
  struct List {
    const std::vector<Buf> *bufs;
    const std::vector<Owned> *recs;
    const uint32_t *order;
    TmRecRef operator[](uint32_t i) const {
      const TmRec &r = (*recs)[order[i]].rec;
      const File f = (*bufs)[r.file].file();
      return TmRecRef{f, tm_before(r.hdr, f.size), r.rlen};
    }
  };
  bool first_rep = true;
  for (uint64_t g = 0; g < groups; ++g) {
    size_t li = 0;
    while (li < logs.size() && logs[li].key != (first_shard + g) % TM_KEYS)
      ++li;
    if (li == logs.size()) continue;
    const auto lo = std::lower_bound(
        order.begin(), order.end(), g,
        [&](uint32_t a, uint64_t q) { return recs[a].q < q; });
    const auto hi = std::lower_bound(
        order.begin(), order.end(), g + 1,
        [&](uint32_t a, uint64_t q) { return recs[a].q < q; });
    const uint32_t n = (uint32_t)(hi - lo);
    const List list{&bufs, &recs, order.data() + (lo - order.begin())};
    lim.shard_id = first_shard + g;
    TrPlan pl;
    MapPlacer mp;
    mp.base = lim.base_index;
    mp.ring.assign(lim.W ? lim.W : 1, 0);
    uint64_t applied = 0;
    uint32_t status = lout[li].status;
    if (status == TRS_OK || status == TRS_TAIL_CUT) {
      pl = tm_validate(list, n, lim);
      status = pl.status;
      if (status == TRS_OK && !tm_replay(list, n, pl, lim, mp, &applied))
        status = TRS_APPLY_STOPPED;
    }
    if (status == TRS_OK) {  // the window pass 2 leaves (as do_replica)
      const uint64_t high = pl.high_index > pl.last_index ? pl.high_index
                                                          : pl.last_index;
      uint64_t lo_i = high + 1 > lim.W ? high + 1 - lim.W : 1;
      if (lo_i > pl.last_index) lo_i = pl.last_index ? pl.last_index : 1;
      if (lo_i <= lim.base_index) lo_i = lim.base_index + 1;
      for (uint64_t i = lo_i; i <= pl.last_index; ++i)
        if (mp.ring[i % mp.ring.size()] != i) status = 100;
    }
    printf("%s%llu~%u %u %llu %llu %llu %llu %llu %llu %llu %llu|",
           first_rep ? "" : ";", (unsigned long long)g, status, pl.files,
           (unsigned long long)pl.offset, (unsigned long long)pl.records,
           (unsigned long long)pl.entries, (unsigned long long)pl.term,
           (unsigned long long)pl.vote, (unsigned long long)pl.commit,
           (unsigned long long)pl.last_index, (unsigned long long)applied);
    first_rep = false;
    bool first = true;
    for (const auto &kv : mp.log) {
      printf("%s%llu/%llu/%s", first ? "" : ",", (unsigned long long)kv.first,
             (unsigned long long)kv.second.first,
             hex(kv.second.second).c_str());
      first = false;
    }
    printf("|");
    for (size_t i = 0; i < mp.applied.size(); ++i)
      printf("%s%llu/%llu", i ? "," : "", (unsigned long long)mp.applied[i],
             (unsigned long long)mp.applied_terms[i]);
  }
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
    if (tok[0] == "index" && tok.size() == 2) do_index(parse(tok[1]));
    else if (tok[0] == "seq" && tok.size() == 2) do_seq(parse(tok[1]));
    else if (tok[0] == "mux" && tok.size() >= 8) do_mux(tok);
    else if (tok[0] == "scan" && tok.size() == 2) do_scan(parse(tok[1]));
    else if (tok[0] == "dump" && tok.size() == 2) do_dump(parse(tok[1]));
    else if (tok[0] == "replica" && tok.size() >= 7) do_replica(tok);
    else return 3;
    if (ch == EOF) break;
  }
  fclose(f);
  return 0;
}
