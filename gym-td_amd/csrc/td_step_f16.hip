// td_step_f16.hip -- the step kernels that write a float16 observation (td_set_obs_format):
// the _f16 variants of td_step.hip's three kernels (see there) and their rows of the launch
// table (step_row_f16).  A unit of its own, so that the two formats compile beside each
// other, not one behind the other.
#include "td_kernels.h"
#include "td_step_body.h"
#include "td_step_launch.h"

namespace td {

// The float16 observation (td_set_obs_format): the same step, the writers instantiated
// for _Float16.  Kernels of their own name, so the float32 kernels keep theirs.
template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) void td_step_kernel_f16(StepArgs a) {
  step_kernel_body<LT, MODE, SCAN, false, _Float16>(a);
}

template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) TD_SMALL_ATTR void td_step_kernel_small_f16(StepArgs a) {
  step_kernel_body<LT, MODE, SCAN, true, _Float16>(kargs(a));
}

#define TD_SMALL2_NAME td_step_kernel_small2_f16
#define TD_SMALL2_OT _Float16
#include "td_step_small2.inc"
#undef TD_SMALL2_NAME
#undef TD_SMALL2_OT

// This unit's rows of the launch table (td_step_launch.h).
template <int LT, int MODE, bool SCAN>
struct F16Kernels {
  static KernelRow large() { return kernel_row(td_step_kernel_f16<LT, MODE, SCAN>, 64, "td_step_kernel_f16"); }
  static KernelRow small() { return kernel_row(td_step_kernel_small_f16<LT, MODE, SCAN>, 64, "td_step_kernel_small_f16"); }
  static KernelRow small2() { return kernel_row(td_step_kernel_small2_f16<LT, MODE, SCAN>, 128, "td_step_kernel_small2_f16"); }
};
static_assert(kObsUnitF16 == ObsFmt<_Float16>::UB, "launch_step's alignment test goes by the float16 store unit");

KernelRow step_row_f16(const StepArgs& a, int kind) { return select_step_row<F16Kernels>(a, kind); }

}  // namespace td
