// drb_launch.hpp -- the step kernel's instantiations as separately compiled
// launchers (drb_step_inst.hip), one per (replicas per group, kind).
#pragma once
#include <hip/hip_runtime.h>

#include "drb_kinds.hpp"
#include "drb_layout.hpp"

namespace drb {

struct RoundParams;  // drb_step.hpp

typedef void (*StepLaunchFn)(const View &v, const RoundParams &p,
                             unsigned grid, hipStream_t s);

#define DRB_STEP_LAUNCH_NAME2(R, K) step_launch_r##R##_k##K
#define DRB_STEP_LAUNCH_NAME(R, K) DRB_STEP_LAUNCH_NAME2(R, K)

// one launcher per kind and R the kind is built for (drb_kinds.hpp)
#define DRB_DECLARE_STEP_LAUNCH(R, K)                                      \
  void DRB_STEP_LAUNCH_NAME(R, K)(const View &v, const RoundParams &p,     \
                                  unsigned grid, hipStream_t s);
#define DRB_X(name, num, kernel, L, E, S, F, LOC, set, alt) \
  DRB_FOR_##set(DRB_DECLARE_STEP_LAUNCH, num)
DRB_STEP_KINDS(DRB_X)
#undef DRB_X

// the tan record kernels (drb_tan.hpp), compiled in drb_tan_inst.hip
void tan_launch_select(const View &v, uint32_t round, uint64_t max_log,
                       uint32_t *list, uint32_t per_list, uint32_t *n,
                       unsigned blocks, hipStream_t s);
void tan_launch_chain(const View &v, uint64_t max_log, unsigned blocks,
                      hipStream_t s);
void tan_launch_write(const View &v, uint32_t round, uint64_t max_log,
                      const uint32_t *list, uint32_t per_list,
                      const uint32_t *n, unsigned blocks, hipStream_t s);

}  // namespace drb
