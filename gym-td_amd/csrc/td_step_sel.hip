// td_step_sel.hip -- the partial-step kernel that writes the float32 observation
// (td_step_sel_kernel: td_step_boards) and its rows of the launch table (sel_row_f32).  The
// body is td_step_sel.h, the step itself td_step_body.h; the float16 kernel is
// td_step_sel_f16.hip.
#include "td_kernels.h"
#include "td_step_launch.h"
#include "td_step_sel.h"

namespace td {

// One wave per named board, grid = the list's length: the large kernel's shape (live slots
// loaded once the header's counts are in, lazy hot record) at any list length.
template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) void td_step_sel_kernel(StepArgs a, const int32_t* ids, int n) {
  step_sel_body<LT, MODE, SCAN>(a, ids, n);
}

// This unit's rows of the launch table (td_step_launch.h): the step kernels' five mode / scan
// rows per side, no small-batch build.
KernelRow sel_row_f32(const StepArgs& a) {
  return select_row(a, [](auto lt, auto mode, auto scan) {
    return kernel_row(td_step_sel_kernel<decltype(lt)::value, decltype(mode)::value, decltype(scan)::value>, 64,
                      "td_step_sel_kernel");
  });
}

}  // namespace td
