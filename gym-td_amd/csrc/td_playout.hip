// td_playout.hip -- the playout kernels (td_playout_kernel) and their rows of the launch table
// (playout_row).  One kernel family serves td_playout, td_playout_boards and
// td_playout_boards_dev: the entries come from PlayoutArgs (td_kernels.h).  The playout itself
// is td_playout.h.  No observation is written, so there is one unit for both formats.
#include "td_kernels.h"
#include "td_playout.h"
#include "td_step_launch.h"

namespace td {

// One wave per entry, several rounds of waves at large batches: the large step kernel's shape
// (no waves-per-SIMD attribute; register and LDS figures in DESIGN.md §4 "Playouts").
template <int LT, int MODE>
__global__ __launch_bounds__(64) void td_playout_kernel(StepArgs a, PlayoutArgs p) {
  playout_kernel_body<LT, MODE>(a, p);  // by value, as td_step_kernel
}

// This unit's rows of the launch table (td_step_launch.h): one kernel per (side, mode).
KernelRow playout_row(const StepArgs& a) {
  return select_row(a, [](auto lt, auto mode, auto) {
    return kernel_row(td_playout_kernel<decltype(lt)::value, decltype(mode)::value>, 64, "td_playout_kernel", kNoScan);
  });
}

}  // namespace td
