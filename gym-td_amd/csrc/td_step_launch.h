// td_step_launch.h -- the host side of a step launch: one table of step kernels for both
// observation formats.  What belongs here: with_side (a run-time map side as a template
// argument, used by every launcher), the table row (StepKernel), its selection from a StepArgs,
// and what is done with a row: launch it, ask its occupancy, print its name.  A step unit names
// its kernels in a template K<LT, MODE, SCAN> with static large() / small() / small2() and
// instantiates the functions below with it; a kernel is compiled where its address is taken.
#pragma once
#include <hip/hip_ext.h>

#include <cstdio>
#include <string>
#include <type_traits>

#include "td_kernels.h"
#include "td_step_obs.h"

namespace td {

// f(std::integral_constant<int, LT>): LT = L where kernels are built for the side, else 0 (generic L).
template <class F>
auto with_side(int L, F&& f) {
  switch (L) {
    case 10: return f(std::integral_constant<int, 10>{});
    case 20: return f(std::integral_constant<int, 20>{});
    case 30: return f(std::integral_constant<int, 30>{});
    default: return f(std::integral_constant<int, 0>{});
  }
}

struct StepKernel {
  void (*fn)(StepArgs);
  int threads;       // per board: 64, or 128 for the two-wave kernel
  const char* name;  // the kernel template, and its arguments (filled in by step_kernel_row):
  int lt = 0, mode = 0;
  bool scan = false;
};

// kind: 0 large, 1 small, 2 small2 (StepArgs::small).  Generic L has the large kernel only.
template <template <int, int, bool> class K, int LT, int MODE, bool SCAN>
StepKernel step_kernel_row(int kind) {
  StepKernel k = K<LT, MODE, SCAN>::large();
  if constexpr (LT != 0) {
    if (kind == 2) k = K<LT, MODE, SCAN>::small2();
    else if (kind != 0) k = K<LT, MODE, SCAN>::small();
  }
  k.lt = LT; k.mode = MODE; k.scan = SCAN;
  return k;
}

// The row of a.L, a.mode and a.multi (SCAN: the multi-action defender scan; TD-atk has none).
template <template <int, int, bool> class K>
StepKernel select_step_kernel(const StepArgs& a, int kind) {
  return with_side(a.L, [&](auto side) {
    constexpr int LT = decltype(side)::value;
    if (a.mode == MODE_ATK) return step_kernel_row<K, LT, MODE_ATK, false>(kind);
    if (a.mode == MODE_DEF) return a.multi ? step_kernel_row<K, LT, MODE_DEF, true>(kind) : step_kernel_row<K, LT, MODE_DEF, false>(kind);
    return a.multi ? step_kernel_row<K, LT, MODE_2P, true>(kind) : step_kernel_row<K, LT, MODE_2P, false>(kind);
  });
}

// Launches a.small's kernel, or the large kernel (its per-element path) where the observation
// is not aligned to the format's store unit.  ev0 / ev1 (optional): timing events bound to the
// step kernel's own dispatch (hipExtLaunchKernelGGL), so their interval is the kernel's
// start-to-end as the dispatch packet timestamps it -- no marker packets around the launch.
template <template <int, int, bool> class K, class OT>
hipError_t launch_step_kernel(const StepArgs& a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  const bool aligned = (reinterpret_cast<uintptr_t>(a.obs) & (ObsFmt<OT>::UB - 1)) == 0;
  const StepKernel k = select_step_kernel<K>(a, aligned ? a.small : 0);
  if (ev0) hipExtLaunchKernelGGL(k.fn, dim3(a.B), dim3(k.threads), 0, s, ev0, ev1, 0, a);
  else hipLaunchKernelGGL(k.fn, dim3(a.B), dim3(k.threads), 0, s, a);
  return hipGetLastError();
}

// Step-kernel workgroups (boards) resident at once on the device: the batch size up to which
// a step runs as one round of waves of the one-wave (waves = 1) or two-wave small-batch kernel.
template <template <int, int, bool> class K>
int step_kernel_resident(const StepArgs& a, int cus, int waves) {
  const StepKernel k = select_step_kernel<K>(a, waves == 2 ? 2 : 1);
  int n = 0;
  if (k.lt == 0) return 0;  // generic-L kernels: no small-batch build
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k.fn, k.threads, 0) == hipSuccess ? n * cus : 0;
}

// The kernel a.small selects, as a profiler prints it: "td_step_kernel_small2<20, 2, true>".
template <template <int, int, bool> class K>
std::string step_kernel_display_name(const StepArgs& a) {
  const StepKernel k = select_step_kernel<K>(a, a.small);
  char buf[96];
  std::snprintf(buf, sizeof buf, "%s<%d, %d, %s>", k.name, k.lt, k.mode, k.scan ? "true" : "false");
  return buf;
}

}  // namespace td
