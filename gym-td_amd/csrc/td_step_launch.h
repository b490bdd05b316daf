// td_step_launch.h -- the host side of a launch: one table for the step, frame-skip and
// partial-step kernels of both observation formats.  What belongs here: with_side (a run-time
// map side as a template argument, used by every launcher), the selection of a table row
// (KernelRow, td_kernels.h) from a StepArgs, and what is done with a row: launch it, ask its
// occupancy, print its name.  A kernel unit supplies only its row for <LT, MODE, SCAN>
// (select_row) and exports that lookup; a kernel is compiled where its address is taken.  The
// rest is ordinary host code, written once and called by td_capi.hip.  No device header is
// included here.
#pragma once
#include <hip/hip_ext.h>

#include <cstdio>
#include <string>
#include <type_traits>

#include "td_kernels.h"

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

// The row of a.L, a.mode and a.multi (SCAN: the multi-action defender scan; TD-atk has none):
// row(lt, mode, scan), three std::integral_constant, returns the family's kernel of those
// template arguments; lt / mode / scan of the row are filled in here.
template <class F>
KernelRow select_row(const StepArgs& a, F&& row) {
  return with_side(a.L, [&](auto lt) {
    auto r = [&](auto mode, auto scan) {
      KernelRow k = row(lt, mode, scan);
      k.lt = decltype(lt)::value;
      k.mode = decltype(mode)::value;
      if (k.scan != kNoScan) k.scan = decltype(scan)::value;
      return k;
    };
    using Def = std::integral_constant<int, MODE_DEF>;
    using Atk = std::integral_constant<int, MODE_ATK>;
    using TwoP = std::integral_constant<int, MODE_2P>;
    if (a.mode == MODE_ATK) return r(Atk{}, std::false_type{});
    if (a.mode == MODE_DEF) return a.multi ? r(Def{}, std::true_type{}) : r(Def{}, std::false_type{});
    return a.multi ? r(TwoP{}, std::true_type{}) : r(TwoP{}, std::false_type{});
  });
}

template <class... A>
KernelRow kernel_row(void (*fn)(A...), int threads, const char* name, int scan = 0) {
  return {reinterpret_cast<const void*>(fn), threads, name, 0, 0, scan};
}

// The step family's row.  A step unit names its kernels in a template K<LT, MODE, SCAN> with
// static large() / small() / small2().  kind: 0 large, 1 small, 2 small2 (StepArgs::small);
// generic L has the large kernel only.  (large, small2, small: the order in which the kernels
// are named here is their order in the unit's code object, and a step kernel is about as large
// as the instruction cache -- with another order the metric's kernel, the same instructions at
// another address, ran 0.9 us of 164 longer, profiles/launch_table.)
template <template <int, int, bool> class K>
KernelRow select_step_row(const StepArgs& a, int kind) {
  return select_row(a, [kind](auto lt, auto mode, auto scan) {
    using T = K<decltype(lt)::value, decltype(mode)::value, decltype(scan)::value>;
    KernelRow k = T::large();
    if constexpr (decltype(lt)::value != 0) {
      if (kind == 2) k = T::small2();
      else if (kind != 0) k = T::small();
    }
    return k;
  });
}

// The four families in the format a.obs_f16.
inline KernelRow step_row(const StepArgs& a, int kind) { return a.obs_f16 ? step_row_f16(a, kind) : step_row_f32(a, kind); }
inline KernelRow skip_row(const StepArgs& a) { return a.obs_f16 ? skip_row_f16(a) : skip_row_f32(a); }
inline KernelRow sel_row(const StepArgs& a) { return a.obs_f16 ? sel_row_f16(a) : sel_row_f32(a); }
inline KernelRow list_row(const StepArgs& a) { return a.obs_f16 ? list_row_f16(a) : list_row_f32(a); }

// One block of k.threads per grid entry; args: the kernel's arguments, in order.  ev0 / ev1
// (optional): timing events bound to the kernel's own dispatch (hipExtLaunchKernel), so their
// interval is the kernel's start-to-end as the dispatch packet timestamps it -- no marker
// packets around the launch (td_kernel_timing).
inline hipError_t launch_row(const KernelRow& k, int grid, void** args, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  if (ev0) (void)hipExtLaunchKernel(k.fn, dim3(grid), dim3(k.threads), args, 0, s, ev0, ev1, 0);
  else (void)hipLaunchKernel(k.fn, dim3(grid), dim3(k.threads), args, 0, s);
  return hipGetLastError();
}

// The observation's store unit per format (td_step_obs.h ObsFmt<OT>::UB; the step units assert it).
constexpr int kObsUnitF32 = 16, kObsUnitF16 = 8;

// The kind a step into a.obs launches where `kind` is asked for: the large kernel (its
// per-element path) where the observation is not aligned to the format's store unit.
inline int step_launch_kind(const StepArgs& a, int kind) {
  const uintptr_t unit = a.obs_f16 ? kObsUnitF16 : kObsUnitF32;
  const bool aligned = (reinterpret_cast<uintptr_t>(a.obs) & (unit - 1)) == 0;
  return aligned ? kind : 0;
}

// The step of this launch's kind (the caller's choice between the handle's two kinds: a launch
// that writes every window, a skipping launch), or of the large kernel for an unaligned buffer.
inline hipError_t launch_step(const StepArgs& a, int kind, hipStream_t s, hipEvent_t ev0 = nullptr,
                              hipEvent_t ev1 = nullptr) {
  void* args[] = {const_cast<StepArgs*>(&a)};
  return launch_row(step_row(a, step_launch_kind(a, kind)), a.B, args, s, ev0, ev1);
}

// Frame skip (a.frame_skip > 1): a.frame_skip board steps per board in one launch of the skip
// kernel of a.L and a.mode.  Discrete actions, random_agent=True only.
inline hipError_t launch_skip(const StepArgs& a, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
  void* args[] = {const_cast<StepArgs*>(&a)};
  return launch_row(skip_row(a), a.B, args, s, ev0, ev1);
}

// Partial step (td_step_boards): one env step for boards ids[0 .. n), n >= 1, every other board
// left as it is; `ids` is device memory, the ids validated by the caller.  One block per list
// entry; the one kernel serves every alignment of the observation (step_board takes the
// per-element writers where the buffer is not aligned for the format).  frame_skip = 1 only.
inline hipError_t launch_step_sel(const StepArgs& a, const int32_t* ids, int n, hipStream_t s, hipEvent_t ev0 = nullptr,
                                  hipEvent_t ev1 = nullptr) {
  void* args[] = {const_cast<StepArgs*>(&a), &ids, &n};
  return launch_row(sel_row(a), n, args, s, ev0, ev1);
}

// The partial step of a device-resident list (td_step_boards_dev): boards ids[0 .. *count) (count ==
// nullptr: cap), unless verdict->code says the check kernel launched in front refused the list.
// One block per entry of cap >= 1: the host does not know the count.
inline hipError_t launch_step_list(const StepArgs& a, const int32_t* ids, int cap, const int32_t* count,
                                   const td_list_status* verdict, hipStream_t s, hipEvent_t ev0 = nullptr,
                                   hipEvent_t ev1 = nullptr) {
  void* args[] = {const_cast<StepArgs*>(&a), &ids, &cap, &count, &verdict};
  return launch_row(list_row(a), cap, args, s, ev0, ev1);
}

// Playouts (td_playout, td_playout_boards[_dev]): a.frame_skip sub-steps for the entries p names,
// one block per entry of `grid` (a.B for every board, the list's n or cap).  Discrete actions,
// random_agent=True only.
inline hipError_t launch_playout(const StepArgs& a, const PlayoutArgs& p, int grid, hipStream_t s,
                                 hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
  void* args[] = {const_cast<StepArgs*>(&a), const_cast<PlayoutArgs*>(&p)};
  return launch_row(playout_row(a), grid, args, s, ev0, ev1);
}

// Probes (td_probe, td_probe_boards[_dev]): q.reps playouts of a.frame_skip sub-steps for each of the
// entries q.p names, one block per (entry, replica) of `entries` (a.B, the list's n or cap).
inline hipError_t launch_probe(const StepArgs& a, const ProbeArgs& q, int entries, hipStream_t s,
                               hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
  const long long grid = (long long)entries * q.reps;
  if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;  // (the kernel's wave index is an int)
  void* args[] = {const_cast<StepArgs*>(&a), const_cast<ProbeArgs*>(&q)};
  return launch_row(probe_row(a), (int)grid, args, s, ev0, ev1);
}

// Small-batch step-kernel workgroups (one per board) resident at once on `cus` compute units:
// the batch size up to which a step runs as one round of waves of the one-wave (waves = 1,
// td_step_kernel_small) or two-wave (td_step_kernel_small2) kernel of the format a.obs_f16.
inline int step_resident_boards(const StepArgs& a, int cus, int waves) {
  const KernelRow k = step_row(a, waves == 2 ? 2 : 1);
  int n = 0;
  if (k.lt == 0) return 0;  // generic-L kernels: no small-batch build
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k.fn, k.threads, 0) == hipSuccess ? n * cus : 0;
}

// A row as a profiler prints it: "td_step_kernel_small2<20, 2, true>", "td_skip_kernel<10, 0>".
inline std::string kernel_display_name(const KernelRow& k) {
  char buf[96];
  if (k.scan == kNoScan) std::snprintf(buf, sizeof buf, "%s<%d, %d>", k.name, k.lt, k.mode);
  else std::snprintf(buf, sizeof buf, "%s<%d, %d, %s>", k.name, k.lt, k.mode, k.scan ? "true" : "false");
  return buf;
}

}  // namespace td
