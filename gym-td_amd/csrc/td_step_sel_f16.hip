// td_step_sel_f16.hip -- the partial-step kernel that writes a float16 observation
// (td_set_obs_format): the _f16 variant of td_step_sel.hip's kernel (see there) with
// launch_step_sel_f16 and step_sel_kernel_name_f16.  A unit of its own, so that the two
// formats compile beside each other, not one behind the other.
#include "td_kernels.h"
#include "td_step_sel.h"

namespace td {

template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) void td_step_sel_kernel_f16(StepArgs a, const int32_t* ids, int n) {
  step_sel_body<LT, MODE, SCAN, _Float16>(a, ids, n);
}

template <int LT, int MODE, bool SCAN>
struct F16Sel {
  static SelKernel sel() { return {td_step_sel_kernel_f16<LT, MODE, SCAN>, "td_step_sel_kernel_f16"}; }
};

hipError_t launch_step_sel_f16(const StepArgs& a, const int32_t* ids, int n, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  return launch_sel_kernel<F16Sel>(a, ids, n, s, ev0, ev1);
}
std::string step_sel_kernel_name_f16(const StepArgs& a) { return sel_kernel_display_name<F16Sel>(a); }

}  // namespace td
