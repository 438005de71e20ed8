// The session table (dragonboat_amd/csrc/drb_session.hpp) as plain C++, for
// tests/test_session_host.py: built with -fsanitize=address,undefined, it
// runs scripts against tables held in heap buffers of exactly the table's
// bytes, through the flat accessor or through rows whose chunks are a stride
// apart (the device layout), and prints every outcome and the exported table.
//
// Script lines:
//   T S H rows            a fresh table (rows 0: flat, 1: strided)
//   A client series responded_to cmd_len value fail
//                         one entry: the decision, then -- unless it is
//                         `full`, or an update whose state machine call the
//                         script lets fail -- the stores
//   X                     the export: client:upto:series=value,...;...
//   I n {client upto n_history {series value}}
//                         an import: OK or ERANGE
// Output: one line per A, X and I line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../dragonboat_amd/csrc/drb_session.hpp"

using namespace drb;

static const char *kNames[] = {"registered",        "register-duplicate",
                               "unregistered",      "unregister-unknown",
                               "unknown-client",    "responded",
                               "cached",            "update",
                               "full"};

namespace {
constexpr uint32_t kStride = 3, kLane = 2;  // rows: the last lane of three
const SessQ kCanary = {0xdeadbeefu, 0xfeedfaceu, 0x0badf00du, 0xcafed00du};

struct Table {
  uint32_t S = 0, H = 0;
  bool rows = false;
  std::vector<SessQ> buf;  // heap: exactly the table's bytes
  uint64_t ops = 0;

  void reset(uint32_t s, uint32_t h, bool r) {
    S = s;
    H = h;
    rows = r;
    ops = 0;
    const size_t chunks = (size_t)S * (2 + H);
    buf.assign(rows ? chunks * kStride : chunks, SessQ{0, 0, 0, 0});
    if (rows)
      for (size_t i = 0; i < buf.size(); ++i)
        if (i % kStride != kLane) buf[i] = kCanary;
  }
  SessFlat<SessQ> flat() { return SessFlat<SessQ>{buf.data()}; }
  SessRows<SessQ> strided() {
    return SessRows<SessQ>{buf.data() + kLane, kStride};
  }
  bool canaries_ok() const {
    if (!rows) return true;
    for (size_t i = 0; i < buf.size(); ++i)
      if (i % kStride != kLane &&
          memcmp(&buf[i], &kCanary, sizeof(SessQ)) != 0)
        return false;
    return true;
  }
};

template <class T>
void apply_line(Table &tb, T t, std::istringstream &in) {
  uint64_t client, series, responded, value;
  uint32_t clen, fail;
  in >> client >> series >> responded >> clen >> value >> fail;
  const std::vector<SessQ> before = tb.buf;
  const SessPlan p =
      sess_decide(t, tb.S, tb.H, client, series, responded, clen);
  const bool failed = p.outcome == SESS_UPDATE && fail;
  if (p.outcome != SESS_FULL && !failed)
    sess_commit(t, tb.H, p, client, series, ++tb.ops + SESS_MAX_SLOTS,
                p.outcome == SESS_UPDATE ? value : 0);
  else if (memcmp(before.data(), tb.buf.data(),
                  before.size() * sizeof(SessQ)) != 0) {
    printf("MISMATCH a refused entry changed the table\n");
    return;
  }
  if (!tb.canaries_ok()) {
    printf("MISMATCH a neighbouring lane was written\n");
    return;
  }
  printf("%s %llu\n", failed ? "update-failed" : kNames[p.outcome],
         (unsigned long long)(p.outcome == SESS_UPDATE ? (failed ? 0 : value)
                                                       : p.value));
}

template <class T>
void export_line(Table &tb, T t) {
  // buffers of exactly the counts: first the counts, then the records
  size_t n = 0, nh = 0;
  sess_export(t, tb.S, tb.H, (SessRec *)nullptr, 0, (SessResp *)nullptr, 0, &n,
              &nh);
  std::vector<SessRec> recs(n);
  std::vector<SessResp> hist(nh);
  size_t n2 = 0, nh2 = 0;
  if (!sess_export(t, tb.S, tb.H, recs.data(), n, hist.data(), nh, &n2,
                   &nh2) ||
      n2 != n || nh2 != nh) {
    printf("MISMATCH export counts\n");
    return;
  }
  std::string out = "X ";
  for (size_t i = 0; i < n; ++i) {
    char b[96];
    snprintf(b, sizeof(b), "%llu:%llu:", (unsigned long long)recs[i].client_id,
             (unsigned long long)recs[i].responded_up_to);
    out += b;
    for (uint32_t h = 0; h < recs[i].n_history; ++h) {
      const SessResp &x = hist[recs[i].first_history + h];
      snprintf(b, sizeof(b), "%s%llu=%llu", h ? "," : "",
               (unsigned long long)x.series_id, (unsigned long long)x.value);
      out += b;
    }
    out += ";";
  }
  printf("%s\n", out.c_str());
}

// I n  then per session: client upto n_history, then its series value pairs
template <class T>
void import_line(Table &tb, T t, std::istringstream &in) {
  size_t n;
  in >> n;
  std::vector<SessRec> recs(n);
  std::vector<SessResp> hist;
  for (size_t i = 0; i < n; ++i) {
    in >> recs[i].client_id >> recs[i].responded_up_to >> recs[i].n_history;
    recs[i].first_history = (uint32_t)hist.size();
    for (uint32_t h = 0; h < recs[i].n_history; ++h) {
      SessResp x;
      in >> x.series_id >> x.value;
      hist.push_back(x);
    }
  }
  const std::vector<SessQ> before = tb.buf;
  const bool ok = sess_import(t, tb.S, tb.H, recs.data(), n, hist.data(),
                              hist.size());
  if (!ok && memcmp(before.data(), tb.buf.data(),
                    before.size() * sizeof(SessQ)) != 0) {
    printf("MISMATCH a refused import changed the table\n");
    return;
  }
  if (!tb.canaries_ok()) {
    printf("MISMATCH a neighbouring lane was written\n");
    return;
  }
  printf("%s\n", ok ? "OK" : "ERANGE");
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream f(argv[1]);
  if (!f) return 2;
  Table tb;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "T") {
      uint32_t s, h, r;
      in >> s >> h >> r;
      if (s < 1 || s > SESS_MAX_SLOTS || h < 1 || h > SESS_MAX_HISTORY)
        return 2;
      tb.reset(s, h, r != 0);
      continue;
    }
    if (tb.buf.empty()) return 2;
    if (op == "A") {
      if (tb.rows)
        apply_line(tb, tb.strided(), in);
      else
        apply_line(tb, tb.flat(), in);
    } else if (op == "X") {
      if (tb.rows)
        export_line(tb, tb.strided());
      else
        export_line(tb, tb.flat());
    } else if (op == "I") {
      if (tb.rows)
        import_line(tb, tb.strided(), in);
      else
        import_line(tb, tb.flat(), in);
    } else if (!op.empty()) {
      return 2;
    }
  }
  return 0;
}
