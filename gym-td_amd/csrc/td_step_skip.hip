// td_step_skip.hip -- the frame-skip kernel that writes the float32 observation
// (td_skip_kernel) and its rows of the launch table (skip_row_f32).  The macro step itself is
// td_step_skip.h; the float16 kernel is td_step_skip_f16.hip.
#include "td_kernels.h"
#include "td_step_launch.h"
#include "td_step_skip.h"

namespace td {

// One wave per board, several rounds of waves at large batches: the large step kernel's
// shape and occupancy (no waves-per-SIMD attribute; register figures in DESIGN.md §4).
template <int LT, int MODE>
__global__ __launch_bounds__(64) void td_skip_kernel(StepArgs a) {
  skip_kernel_body<LT, MODE, float>(a);  // by value, as td_step_kernel
}

// This unit's rows of the launch table (td_step_launch.h): one kernel per (side, mode).
KernelRow skip_row_f32(const StepArgs& a) {
  return select_row(a, [](auto lt, auto mode, auto) {
    return kernel_row(td_skip_kernel<decltype(lt)::value, decltype(mode)::value>, 64, "td_skip_kernel", kNoScan);
  });
}

}  // namespace td
