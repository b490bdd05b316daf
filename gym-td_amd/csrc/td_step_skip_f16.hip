// td_step_skip_f16.hip -- the frame-skip kernel that writes a float16 observation
// (td_skip_kernel_f16) with launch_skip_f16 and skip_kernel_name_f16.  A unit of its own,
// so that the two formats compile beside each other (as td_step_f16.hip).
#include "td_kernels.h"
#include "td_step_skip.h"

namespace td {

template <int LT, int MODE>
__global__ __launch_bounds__(64) void td_skip_kernel_f16(StepArgs a) {
  skip_kernel_body<LT, MODE, _Float16>(a);
}

template <int LT, int MODE>
struct F16Skip {
  static auto fn() { return td_skip_kernel_f16<LT, MODE>; }
  static const char* name() { return "td_skip_kernel_f16"; }
};

hipError_t launch_skip_f16(const StepArgs& a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  return launch_skip_kernel<F16Skip>(a, s, ev0, ev1);
}
std::string skip_kernel_name_f16(const StepArgs& a) { return skip_kernel_display_name<F16Skip>(a); }

}  // namespace td
