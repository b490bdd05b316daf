// td_step_list_f16.hip -- the partial-step kernel of a device-resident list that writes a
// float16 observation (td_set_obs_format): the _f16 variant of td_step_list.hip's kernel (see
// there) and its rows of the launch table (list_row_f16).  A unit of its own, so that the two
// formats compile beside each other.
#include "td_kernels.h"
#include "td_step_launch.h"
#include "td_step_list.h"

namespace td {

template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) void td_step_list_kernel_f16(StepArgs a, const int32_t* ids, int cap,
                                                              const int32_t* count, const td_list_status* verdict) {
  step_list_body<LT, MODE, SCAN, _Float16>(a, ids, cap, count, verdict);
}

KernelRow list_row_f16(const StepArgs& a) {
  return select_row(a, [](auto lt, auto mode, auto scan) {
    return kernel_row(td_step_list_kernel_f16<decltype(lt)::value, decltype(mode)::value, decltype(scan)::value>, 64,
                      "td_step_list_kernel_f16");
  });
}

}  // namespace td
