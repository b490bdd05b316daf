// td_mask.hip -- legal-action masks of every board's present state (td_action_mask).
//
// One wave per board, as the step, one board per workgroup; the board's work is
// td_mask_body.h's mask_board, shared with the list form (td_mask_list.hip).
#include "td_mask_body.h"

namespace td {

template <int LT>
__global__ __launch_bounds__(64) void td_mask_kernel(MaskArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t R[MaskRow<LT>::BYTES];
  const int i = blockIdx.x, lane = (int)threadIdx.x;
  if (i >= a.B) return;
  mask_board<LT>(a, a.xcd_map ? xcd_board(i, a.B) : i, lane, R);
}

hipError_t launch_mask(const MaskArgs& a, hipStream_t s) {
  switch (a.L) {
    case 10: hipLaunchKernelGGL(td_mask_kernel<10>, dim3(a.B), dim3(64), 0, s, a); break;
    case 20: hipLaunchKernelGGL(td_mask_kernel<20>, dim3(a.B), dim3(64), 0, s, a); break;
    case 30: hipLaunchKernelGGL(td_mask_kernel<30>, dim3(a.B), dim3(64), 0, s, a); break;
    default: hipLaunchKernelGGL(td_mask_kernel<0>, dim3(a.B), dim3(64), 0, s, a); break;
  }
  return hipGetLastError();
}

}  // namespace td
