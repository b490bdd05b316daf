// td_copy_list.hip -- td_copy_list_kernel: the board copy of a device-resident list
// (td_copy_boards_dev).  td_copy_kernel's body (td_copy_body.h) behind a prologue that makes the
// pair count of two words in device memory: the count (or cap, where the caller gave none) and
// the verdict of the check kernel launched in front (td_list_check.hip).  A refused list is one
// of no pairs: every wave exits before it reads an id or anything of any board.  A unit of its
// own: see td_copy_body.h.
#include "td_copy_body.h"
#include "td_list_dev.h"

namespace td {

// src / dst: [cap] board ids; count: [1] or nullptr; verdict: the handle's record.  The pair
// count is td_list_dev.h's dev_list_length: n <= cap = the grid, and entries [0, n) were all
// validated.
template <int LT>
__global__ __launch_bounds__(64) void td_copy_list_kernel(StepArgs a, const int32_t* src, const int32_t* dst, int cap,
                                                          const int32_t* count, const td_list_status* verdict) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ Smem<NC> S;
  const int n = dev_list_length(cap, count, verdict);
  TD_COPY_PAIR_BODY(src[i], dst[i])
}

hipError_t launch_copy_list(const StepArgs& a, const int32_t* src, const int32_t* dst, int cap, const int32_t* count,
                            const td_list_status* verdict, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  with_side(a.L, [&](auto lt) {
    auto k = td_copy_list_kernel<decltype(lt)::value>;
    if (ev0) hipExtLaunchKernelGGL(k, dim3(cap), dim3(64), 0, s, ev0, ev1, 0, a, src, dst, cap, count, verdict);
    else hipLaunchKernelGGL(k, dim3(cap), dim3(64), 0, s, a, src, dst, cap, count, verdict);
  });
  return hipGetLastError();
}

}  // namespace td
