// td_step_skip.hip -- the frame-skip kernel that writes the float32 observation
// (td_skip_kernel) with launch_skip and skip_kernel_name.  The macro step itself is
// td_step_skip.h; the float16 kernel is td_step_skip_f16.hip.
#include "td_kernels.h"
#include "td_step_skip.h"

namespace td {

// One wave per board, several rounds of waves at large batches: the large step kernel's
// shape and occupancy (no waves-per-SIMD attribute; register figures in DESIGN.md §4).
template <int LT, int MODE>
__global__ __launch_bounds__(64) void td_skip_kernel(StepArgs a) {
  skip_kernel_body<LT, MODE, float>(a);  // by value, as td_step_kernel
}

template <int LT, int MODE>
struct F32Skip {
  static auto fn() { return td_skip_kernel<LT, MODE>; }
  static const char* name() { return "td_skip_kernel"; }
};

hipError_t launch_skip(const StepArgs& a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  return a.obs_f16 ? launch_skip_f16(a, s, ev0, ev1) : launch_skip_kernel<F32Skip>(a, s, ev0, ev1);
}
std::string skip_kernel_name(const StepArgs& a) {
  return a.obs_f16 ? skip_kernel_name_f16(a) : skip_kernel_display_name<F32Skip>(a);
}

}  // namespace td
