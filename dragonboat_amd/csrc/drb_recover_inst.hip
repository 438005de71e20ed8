// drb_recover_inst.hip -- the recovery kernels (drb_recover.hpp) and their
// launchers, a translation unit of their own (dragonboat_amd/build.py): the
// step kernels' units are not touched by them, and the engine's host code
// does not wait on their register allocation.
//
// Written for gfx950 (MI355X) only.
#include <hip/hip_runtime.h>

#define DRB_RECOVER_KERNELS 1
#include "drb_recover.hpp"

namespace drb {

void recover_launch_check(const View &v, const RecParams &p, unsigned blocks,
                          hipStream_t s) {
  k_recover_check<<<blocks, REC_BLOCK, 0, s>>>(v, p);
}

void recover_launch_place(const View &v, const RecParams &p, unsigned blocks,
                          hipStream_t s) {
  k_recover_place<<<blocks, REC_BLOCK, 0, s>>>(v, p);
}

}  // namespace drb
