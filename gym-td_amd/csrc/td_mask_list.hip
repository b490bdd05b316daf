// td_mask_list.hip -- td_mask_list_kernel: legal-action masks of the boards a list names
// (td_action_mask_boards, td_action_mask_boards_dev).  The board's work is td_mask_body.h's
// mask_board, the one td_mask_kernel runs: row b of every output comes out byte for byte as
// td_action_mask writes it, and no byte of any other row is stored (the 16-B pieces a row
// shares with its neighbours go out byte by byte there).
//
// Shape: one wave per list entry, kMaskListWaves entries per workgroup, consecutive entries in
// one workgroup -- a sorted run of neighbouring boards assembles the lines its rows share in
// one L2, and a list costs a quarter of the workgroups td_mask_kernel's shape would.  Each wave
// has its own LDS row and orders its accesses with wsync() alone: no workgroup barrier, so the
// waves of a partial last workgroup and of a shortened list simply return.
#include "td_mask_body.h"

namespace td {

// ids: [cap] board ids in device memory.  Host-list form: verdict == nullptr, the ids were
// validated on the host and cap entries are used.  Device-list form: count ([1] or nullptr = cap)
// and verdict (the handle's record); a refused list has length 0 and every wave exits before it
// reads an id (td_list_dev.h: the length, the wave's entry, the id as a scalar load).
template <int LT>
__global__ __launch_bounds__(64 * kMaskListWaves) void td_mask_list_kernel(MaskArgs a, const int32_t* ids, int cap,
                                                                            const int32_t* count,
                                                                            const td_list_status* verdict) {
  constexpr int RB = MaskRow<LT>::BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t R[kMaskListWaves][RB];
  static_assert(RB % 16 == 0, "every wave's row is 16-B aligned");
  const int n = list_length(cap, count, verdict);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  int i;
  if (!list_wave_entry<kMaskListWaves>(a.v.xcd_map, n, wave, &i)) return;
  const int b = list_word(ids, i);
  mask_board<LT>(a, b, lane, R[wave]);
}

hipError_t launch_mask_list(const MaskArgs& a, const int32_t* ids, int cap, const int32_t* count,
                            const td_list_status* verdict, hipStream_t s) {
  const dim3 grid((cap + kMaskListWaves - 1) / kMaskListWaves), block(64 * kMaskListWaves);
  with_side(a.v.L, [&](auto lt) {
    hipLaunchKernelGGL(td_mask_list_kernel<decltype(lt)::value>, grid, block, 0, s, a, ids, cap, count, verdict);
  });
  return hipGetLastError();
}

}  // namespace td
