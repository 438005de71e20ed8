// The stand-alone program of tests/test_snappy_host.py: drb_snappy.hpp on the
// CPU, built with -fsanitize=address,undefined.
//
//   snappy_host_main VECTORS
// VECTORS holds one vector per line, "<cap> <hex of the Cmd, or ->".  For
// each the program prints the payload in hex ("-" when empty), or ERR.
// Every Cmd is decoded twice -- through the flat accessors (payload_decode,
// what drb_payload_decode runs) and, when it is a Snappy one and cap is a
// multiple of 16, through the 16 B-chunk rows the device uses, with input
// and output buffers of exactly the bytes the decoder may touch, so that the
// sanitizer sees any access outside them.  MISMATCH is printed if the two
// disagree.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../dragonboat_amd/csrc/drb_snappy.hpp"

struct alignas(16) Q16 {
  uint32_t x, y, z, w;
};

static const uint64_t STRIDE = 3;  // chunks between a row's chunks

static int hexval(int c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

// 0 and the payload, or nonzero
static int decode_rows(const std::vector<uint8_t> &cmd, size_t cap,
                       std::vector<uint8_t> &out) {
  const size_t nq = (cmd.size() + 15) / 16, dq = cap / 16;
  std::vector<Q16> in((nq - 1) * STRIDE + 1), row((dq - 1) * STRIDE + 1);
  for (size_t i = 0; i < cmd.size(); ++i)
    ((uint8_t *)&in[(i / 16) * STRIDE])[i % 16] = cmd[i];
  // the row starts full of another payload's bytes
  memset(row.data(), 0xee, row.size() * sizeof(Q16));
  drb::SnapRowsIn<Q16> si(in.data(), STRIDE);
  drb::SnapRowsOut<Q16> so(row.data(), STRIDE);
  uint32_t n = 0;
  const int rc =
      drb::snappy_decode(si, (uint32_t)cmd.size(), so, (uint32_t)cap, &n);
  if (rc) return rc;
  out.resize(n);
  for (size_t i = 0; i < n; ++i)
    out[i] = ((const uint8_t *)&row[(i / 16) * STRIDE])[i % 16];
  // zeros up to the end of the last chunk (SnapRowsOut::finish)
  for (size_t i = n; i % 16; ++i)
    if (((const uint8_t *)&row[(i / 16) * STRIDE])[i % 16]) return 100;
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<char> line(1 << 16);
  while (fgets(line.data(), (int)line.size(), f)) {
    char *sp = strchr(line.data(), ' ');
    if (!sp) return 3;
    const size_t cap = strtoul(line.data(), nullptr, 10);
    std::vector<uint8_t> cmd;
    for (const char *p = sp + 1; hexval(p[0]) >= 0 && hexval(p[1]) >= 0; p += 2)
      cmd.push_back((uint8_t)(hexval(p[0]) * 16 + hexval(p[1])));
    // exactly cap bytes: a write past the capacity is a heap overflow
    std::vector<uint8_t> out(cap);
    size_t n = 0;
    const int rc = drb::payload_decode(2 /*ENCODED*/, cmd.data(), cmd.size(),
                                       out.data(), cap, &n);
    bool same = true;
    if (cmd.size() > 1 && cmd[0] == 0x02 && cap && cap % 16 == 0) {
      std::vector<uint8_t> out2;
      const int rc2 = decode_rows(cmd, cap, out2);
      same = (rc == 0) == (rc2 == 0) &&
             (rc || (out2.size() == n &&
                     (n == 0 || !memcmp(out2.data(), out.data(), n))));
    }
    if (!same) {
      puts("MISMATCH");
    } else if (rc) {
      puts("ERR");
    } else if (n == 0) {
      puts("-");
    } else {
      std::string s;
      for (size_t i = 0; i < n; ++i) {
        char b[3];
        snprintf(b, sizeof b, "%02x", out[i]);
        s += b;
      }
      puts(s.c_str());
    }
  }
  fclose(f);
  return 0;
}
