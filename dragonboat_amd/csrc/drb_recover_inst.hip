// drb_recover_inst.hip -- the recovery kernels (drb_recover.hpp, and
// drb_recover_mux.hpp for the multiplexed tan logs) and their launchers, a
// translation unit of their own (dragonboat_amd/build.py): the step kernels'
// units are not touched by them, and the engine's host code does not wait on
// their register allocation.  The scan and the sort of the multiplexed
// recovery (hipCUB) are instantiated here as well.
//
// Written for gfx950 (MI355X) only.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#define DRB_RECOVER_KERNELS 1
#include "drb_recover.hpp"
#include "drb_recover_mux.hpp"

namespace drb {

void recover_launch_check(const View &v, const RecParams &p, unsigned blocks,
                          hipStream_t s) {
  k_recover_check<<<blocks, REC_BLOCK, 0, s>>>(v, p);
}

void recover_launch_place(const View &v, const RecParams &p, unsigned blocks,
                          hipStream_t s) {
  k_recover_place<<<blocks, REC_BLOCK, 0, s>>>(v, p);
}

// ------------------------------------------------------------ multiplexed
static unsigned mux_grid(uint64_t lanes) {
  return (unsigned)((lanes + REC_BLOCK - 1) / REC_BLOCK);
}

// the bits of the sort key: q < bound
static int mux_bits(uint64_t bound) {
  int bits = 1;
  while (bits < 32 && (1ull << bits) < bound) bits++;
  return bits;
}

void recover_mux_index(const View &v, const MuxParams &p, hipStream_t s) {
  (void)v;
  if (p.n_blocks) k_mux_index<<<mux_grid(p.n_blocks), REC_BLOCK, 0, s>>>(p);
  k_mux_compose<<<mux_grid(p.n_logs), REC_BLOCK, 0, s>>>(p);
}

size_t recover_mux_scan_temp(uint32_t n) {
  size_t tb = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t *)nullptr,
                                         (uint32_t *)nullptr, (int)n);
  return tb;
}

hipError_t recover_mux_scan(const MuxParams &p, void *tmp, size_t tmp_bytes,
                            hipStream_t s) {
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, p.cnt, p.first,
                                          (int)p.n_blocks, s);
}

void recover_mux_records(const View &v, const MuxParams &p, hipStream_t s) {
  k_mux_records<<<mux_grid(p.n_blocks), REC_BLOCK, 0, s>>>(v, p);
}

size_t recover_mux_sort_temp(uint32_t n, uint64_t bound) {
  size_t tb = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(
      nullptr, tb, (uint32_t *)nullptr, (uint32_t *)nullptr,
      (uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, mux_bits(bound));
  return tb;
}

hipError_t recover_mux_sort(const MuxParams &p, uint32_t *keys_out,
                            uint32_t *vals_out, uint64_t bound, void *tmp,
                            size_t tmp_bytes, hipStream_t s) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, p.keys, keys_out,
                                            p.vals, vals_out, (int)p.n_recs, 0,
                                            mux_bits(bound), s);
}

void recover_mux_check(const View &v, const MuxParams &p, hipStream_t s) {
  const uint64_t lanes = v.G * v.R > p.n_logs ? v.G * v.R : p.n_logs;
  k_mux_check<<<mux_grid(lanes), REC_BLOCK, 0, s>>>(v, p);
}

void recover_mux_place(const View &v, const MuxParams &p, hipStream_t s) {
  const uint64_t lanes = v.G * v.R > p.n_logs ? v.G * v.R : p.n_logs;
  k_mux_place<<<mux_grid(lanes), REC_BLOCK, 0, s>>>(v, p);
}

}  // namespace drb
