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
// and verdict (the handle's record) were written by earlier kernels on the stream and by no
// wave of this one, so they are wave-uniform loads through the constant address space, as in
// td_step_list.h; a refused list has length 0 and every wave exits before it reads an id.  The
// check kernel refused a count outside [0, cap], so n <= cap and ids[0 .. n) were validated.
template <int LT>
__global__ __launch_bounds__(64 * kMaskListWaves) void td_mask_list_kernel(MaskArgs a, const int32_t* ids, int cap,
                                                                            const int32_t* count,
                                                                            const td_list_status* verdict) {
  constexpr int RB = MaskRow<LT>::BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t R[kMaskListWaves][RB];
  static_assert(RB % 16 == 0, "every wave's row is 16-B aligned");
  typedef __attribute__((address_space(4))) const int32_t cword_t;
  int n = cap;
  if (verdict) {
    const int code = reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(verdict))[0];
    static_assert(offsetof(td_list_status, code) == 0, "the verdict's first word");
    if (count) n = reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(count))[0];
    n = code ? 0 : n;
  }
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  // workgroup g of the grid serves group xcd_board(g, groups) of kMaskListWaves consecutive
  // entries: consecutive groups on one XCD, as the partial step places consecutive entries
  const int groups = (n + kMaskListWaves - 1) / kMaskListWaves, g = (int)blockIdx.x;
  if (g >= groups) return;
  const int i = (a.xcd_map ? xcd_board(g, groups) : g) * kMaskListWaves + wave;
  if (i >= n) return;
  // the id: a scalar load beside the argument loads (td_step_sel.h says why not a vector load)
  const int b = reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(ids))[i];
  mask_board<LT>(a, b, lane, R[wave]);
}

hipError_t launch_mask_list(const MaskArgs& a, const int32_t* ids, int cap, const int32_t* count,
                            const td_list_status* verdict, hipStream_t s) {
  const dim3 grid((cap + kMaskListWaves - 1) / kMaskListWaves), block(64 * kMaskListWaves);
  switch (a.L) {
    case 10: hipLaunchKernelGGL(td_mask_list_kernel<10>, grid, block, 0, s, a, ids, cap, count, verdict); break;
    case 20: hipLaunchKernelGGL(td_mask_list_kernel<20>, grid, block, 0, s, a, ids, cap, count, verdict); break;
    case 30: hipLaunchKernelGGL(td_mask_list_kernel<30>, grid, block, 0, s, a, ids, cap, count, verdict); break;
    default: hipLaunchKernelGGL(td_mask_list_kernel<0>, grid, block, 0, s, a, ids, cap, count, verdict); break;
  }
  return hipGetLastError();
}

}  // namespace td
