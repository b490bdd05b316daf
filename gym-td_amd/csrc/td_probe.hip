// td_probe.hip -- the probe kernels (td_probe_kernel) and their rows of the launch table
// (probe_row).  One kernel family serves td_probe, td_probe_boards and td_probe_boards_dev: the
// entries and the replicas come from ProbeArgs (td_kernels.h).  The probe itself is td_probe.h
// over td_playout.h's sub-steps.  No observation is written, so there is one unit for both formats.
#include "td_kernels.h"
#include "td_probe.h"
#include "td_step_launch.h"

namespace td {

// One wave per (entry, replica), several rounds of waves: the playout kernel's shape (no
// waves-per-SIMD attribute; register and LDS figures in DESIGN.md §4 "Probes").
template <int LT, int MODE>
__global__ __launch_bounds__(64) void td_probe_kernel(StepArgs a, ProbeArgs q) {
  probe_kernel_body<LT, MODE>(a, q);  // by value, as td_step_kernel
}

// This unit's rows of the launch table (td_step_launch.h): one kernel per (side, mode).
KernelRow probe_row(const StepArgs& a) {
  return select_row(a, [](auto lt, auto mode, auto) {
    return kernel_row(td_probe_kernel<decltype(lt)::value, decltype(mode)::value>, 64, "td_probe_kernel", kNoScan);
  });
}

}  // namespace td
