// td_step.hip -- the step kernels that write the float32 observation (td_step_kernel,
// td_step_kernel_small, td_step_kernel_small2) and their rows of the launch table
// (step_row_f32).  The step itself is td_step_body.h; the float16 kernels are
// td_step_f16.hip; the reset, refill and opponent kernels td_reset.hip.
#include "td_kernels.h"
#include "td_step_body.h"
#include "td_step_launch.h"

namespace td {

// Large batches (several rounds of waves, HBM-write bound): 6 waves per SIMD at
// L = 10 (106 SGPRs), no register pressure beyond the step's own.
template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) void td_step_kernel(StepArgs a) {
  step_kernel_body<LT, MODE, SCAN, false>(a);  // by value (see kargs)
}

// Batches that fit one round of waves.  8 waves per SIMD where LDS allows it (L = 10:
// 5,072 B per board): the compiler then keeps the kernel at <= 80 SGPRs, the gfx950
// limit for 8 resident waves (MI355X_MICROARCH.md, residency), so 8,192 boards -- 8
// GPUs' share of BASELINE's 65,536 -- run as ONE round instead of 6,144 + 2,048.  At
// 65,536 boards the same build is 7 % slower (SGPR spill code), hence two kernels.
template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) TD_SMALL_ATTR void td_step_kernel_small(StepArgs a) {
  step_kernel_body<LT, MODE, SCAN, true>(kargs(a));
}

// Batches up to half the resident waves: two waves per board.  The first steps the board
// as in td_step_kernel_small; the second waits at one barrier and writes the second half
// of the observation windows beside it, which shortens a board's critical path where the
// batch leaves issue slots free (4,096 boards: 8,192 waves, 8 per SIMD).
#define TD_SMALL2_NAME td_step_kernel_small2
#define TD_SMALL2_OT float
#include "td_step_small2.inc"
#undef TD_SMALL2_NAME
#undef TD_SMALL2_OT

// This unit's rows of the launch table (td_step_launch.h).
template <int LT, int MODE, bool SCAN>
struct F32Kernels {
  static KernelRow large() { return kernel_row(td_step_kernel<LT, MODE, SCAN>, 64, "td_step_kernel"); }
  static KernelRow small() { return kernel_row(td_step_kernel_small<LT, MODE, SCAN>, 64, "td_step_kernel_small"); }
  static KernelRow small2() { return kernel_row(td_step_kernel_small2<LT, MODE, SCAN>, 128, "td_step_kernel_small2"); }
};
static_assert(kObsUnitF32 == ObsFmt<float>::UB, "launch_step's alignment test goes by the float32 store unit");

KernelRow step_row_f32(const StepArgs& a, int kind) { return select_step_row<F32Kernels>(a, kind); }

}  // namespace td
