// td_copy.hip -- td_copy_kernel: boards dst[i] become exact copies of boards src[i] of the same
// handle (td_copy_boards), one wave per pair, between two steps on the step's stream.
//
// State travels as raw 16-B words of the per-board slices, never through load_board /
// store_board: store_board writes the tower words and the header's second half only on the
// steps that changed them, and a clone needs them always.  The header goes first; its counts
// bound the slot copies, whose loads are all issued before the first store.  Epoch tags travel
// as they are: both boards read the handle's constant blocks, and td_cfg_usage_kernel counts
// the clone's entities like any other board's.
//
// The observation is no copy of the source's row (the caller's buffer may hold anything there):
// the *source* board is staged in LDS as td_opponent_kernel stages it, the group statistics and
// broadcast channels are derived as at the end of a step, and every window of the
// destination's row is written by the step's own writers -- what a full write of that state
// under the current constant block leaves: bytewise what the step that produced the state
// wrote, unless td_set_config came between (progress, the cost bits and the e_cost channels
// read the current block; the next step rewrites those classes either way).  One build per map side serves both observation formats
// (a.obs_f16 is a run-time branch, as in reset_one): a copy is no step's hot path.
//
// The body of a pair is td_copy_body.h's, shared with td_copy_list_kernel (td_copy_list.hip:
// td_copy_boards_dev, the lists in device memory).
#include "td_copy_body.h"

namespace td {

// pairs: [2 n] board ids, the sources then the destinations (validated on the host: every id
// in [0, B), no destination named twice, none that is also a source).
template <int LT>
__global__ __launch_bounds__(64) void td_copy_kernel(StepArgs a, const int32_t* pairs, int n) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ Smem<NC> S;
  TD_COPY_PAIR_BODY(pairs[i], pairs[n + i])
}

hipError_t launch_copy(const StepArgs& a, const int32_t* pairs, int n, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  with_side(a.L, [&](auto lt) {
    if (ev0) hipExtLaunchKernelGGL(td_copy_kernel<decltype(lt)::value>, dim3(n), dim3(64), 0, s, ev0, ev1, 0, a, pairs, n);
    else hipLaunchKernelGGL(td_copy_kernel<decltype(lt)::value>, dim3(n), dim3(64), 0, s, a, pairs, n);
  });
  return hipGetLastError();
}

}  // namespace td
