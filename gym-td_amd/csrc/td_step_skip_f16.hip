// td_step_skip_f16.hip -- the frame-skip kernel that writes a float16 observation
// (td_skip_kernel_f16) and its rows of the launch table (skip_row_f16).  A unit of its own,
// so that the two formats compile beside each other (as td_step_f16.hip).
#include "td_kernels.h"
#include "td_step_launch.h"
#include "td_step_skip.h"

namespace td {

template <int LT, int MODE>
__global__ __launch_bounds__(64) void td_skip_kernel_f16(StepArgs a) {
  skip_kernel_body<LT, MODE, _Float16>(a);
}

KernelRow skip_row_f16(const StepArgs& a) {
  return select_row(a, [](auto lt, auto mode, auto) {
    return kernel_row(td_skip_kernel_f16<decltype(lt)::value, decltype(mode)::value>, 64, "td_skip_kernel_f16", kNoScan);
  });
}

}  // namespace td
