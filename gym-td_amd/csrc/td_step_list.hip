// td_step_list.hip -- the partial-step kernel of a device-resident list that writes the
// float32 observation (td_step_list_kernel: td_step_boards_dev) and its rows of the launch
// table (list_row_f32).  The body is td_step_list.h, the step itself td_step_sel.h /
// td_step_body.h; the float16 kernel is td_step_list_f16.hip.
#include "td_kernels.h"
#include "td_step_launch.h"
#include "td_step_list.h"

namespace td {

// One wave per list entry, grid = cap (the host does not know the count): td_step_sel_kernel's
// shape, its length read on the device.
template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) void td_step_list_kernel(StepArgs a, const int32_t* ids, int cap, const int32_t* count,
                                                          const td_list_status* verdict) {
  step_list_body<LT, MODE, SCAN>(a, ids, cap, count, verdict);
}

// This unit's rows of the launch table (td_step_launch.h): the same five mode / scan rows per
// side as sel_row_f32.
KernelRow list_row_f32(const StepArgs& a) {
  return select_row(a, [](auto lt, auto mode, auto scan) {
    return kernel_row(td_step_list_kernel<decltype(lt)::value, decltype(mode)::value, decltype(scan)::value>, 64,
                      "td_step_list_kernel");
  });
}

}  // namespace td
