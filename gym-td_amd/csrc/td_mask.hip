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
  if (i >= a.v.B) return;
  mask_board<LT>(a, a.v.xcd_map ? xcd_board(i, a.v.B) : i, lane, R);
}

hipError_t launch_mask(const MaskArgs& a, hipStream_t s) {
  with_side(a.v.L, [&](auto lt) {
    hipLaunchKernelGGL(td_mask_kernel<decltype(lt)::value>, dim3(a.v.B), dim3(64), 0, s, a);
  });
  return hipGetLastError();
}

}  // namespace td
