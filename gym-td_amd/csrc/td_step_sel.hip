// td_step_sel.hip -- the partial-step kernel that writes the float32 observation
// (td_step_sel_kernel: td_step_boards) with launch_step_sel and step_sel_kernel_name.  The
// body is td_step_sel.h, the step itself td_step_body.h; the float16 kernel is
// td_step_sel_f16.hip.
#include "td_kernels.h"
#include "td_step_sel.h"

namespace td {

// One wave per named board, grid = the list's length: the large kernel's shape (live slots
// loaded once the header's counts are in, lazy hot record) at any list length.
template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(64) void td_step_sel_kernel(StepArgs a, const int32_t* ids, int n) {
  step_sel_body<LT, MODE, SCAN>(a, ids, n);
}

template <int LT, int MODE, bool SCAN>
struct F32Sel {
  static SelKernel sel() { return {td_step_sel_kernel<LT, MODE, SCAN>, "td_step_sel_kernel"}; }
};

hipError_t launch_step_sel(const StepArgs& a, const int32_t* ids, int n, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  return a.obs_f16 ? launch_step_sel_f16(a, ids, n, s, ev0, ev1) : launch_sel_kernel<F32Sel>(a, ids, n, s, ev0, ev1);
}
std::string step_sel_kernel_name(const StepArgs& a) {
  return a.obs_f16 ? step_sel_kernel_name_f16(a) : sel_kernel_display_name<F32Sel>(a);
}

}  // namespace td
