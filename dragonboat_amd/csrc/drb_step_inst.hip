// drb_step_inst.hip -- one instantiation of the step kernel (drb_step.hpp)
// and its launcher, compiled once per (R, kind) with -DDRB_INST_R and
// -DDRB_INST_KIND (dragonboat_amd/build.py), the kind's template arguments
// read from the kinds table (drb_kinds.hpp).  The instantiations are
// independent translation units so the build runs them in parallel; the
// engine (drb_engine.hip) calls them through kStepLaunch.
//
// Written for gfx950 (MI355X) only.
#include <hip/hip_runtime.h>

#include "drb_launch.hpp"
#include "drb_step.hpp"

#ifndef DRB_INST_R
#error "DRB_INST_R (replicas per group) is required"
#endif
#ifndef DRB_INST_KIND
#error "DRB_INST_KIND (drb_kinds.hpp StepKind) is required"
#endif

namespace drb {

void DRB_STEP_LAUNCH_NAME(DRB_INST_R, DRB_INST_KIND)(const View &v,
                                                     const RoundParams &p,
                                                     unsigned grid,
                                                     hipStream_t s) {
  constexpr StepKindInfo K = kStepKinds[DRB_INST_KIND];
  if constexpr (K.kernel == SKN_LEAN) {
    lean_kernel<DRB_INST_R, K.lead><<<grid, 256, 0, s>>>(v, p);
  } else {
    // the leader's per-remote entry-row floors (LDS) exist with placement C4
    const size_t dyn =
        K.lead && !K.local && v.remote_mask ? DRB_INST_R * 256 * 8 : 0;
    step_kernel<DRB_INST_R, K.lead, K.ext, K.slow, K.fwd, K.local>
        <<<grid, 256, dyn, s>>>(v, p);
  }
}

}  // namespace drb
