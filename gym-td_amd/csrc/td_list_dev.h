// td_list_dev.h -- what the kernels that serve a board list read of it, each written once: a
// word of it through the constant address space, the list's length, and the entry a wave of a
// wave-per-entry kernel serves.  Device text only.
//
// A list's ids, its count and the handle's verdict were written by earlier kernels (or copies)
// on the stream and by no wave of the kernel that reads them, and the kernel boundary makes them
// visible: wave-uniform SMEM loads beside the argument loads (td_step_sel.h says why not vector
// loads).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "td_kernels.h"

namespace td {

__device__ __forceinline__ int list_word(const int32_t* p, int i = 0) {
  typedef __attribute__((address_space(4))) const int32_t cword_t;
  return reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(p))[i];
}

// The length of a device-resident list: the count (or cap, where the caller gave none), and 0
// where verdict->code says the check kernel launched in front (td_list_check.hip) refused the
// list -- then every wave exits before it reads an id or anything of any board.  The check
// kernel refused a count outside [0, cap], so n <= cap and entries [0, n) were all validated.
__device__ __forceinline__ int dev_list_length(int cap, const int32_t* count, const td_list_status* verdict) {
  const int code = list_word(reinterpret_cast<const int32_t*>(verdict));
  static_assert(offsetof(td_list_status, code) == 0, "the verdict's first word");
  int n = cap;
  if (count) n = list_word(count);
  n = code ? 0 : n;
  return n;
}

// The same where a kernel serves host lists too: verdict == nullptr, the ids were validated on
// the host and cap entries are used.
__device__ __forceinline__ int list_length(int cap, const int32_t* count, const td_list_status* verdict) {
  return verdict ? dev_list_length(cap, count, verdict) : cap;
}

// The map of the wave-per-entry kernels, WAVES entries per workgroup: workgroup g of the grid
// serves group xcd_board(g, groups) of WAVES consecutive entries (consecutive groups on one XCD,
// as the partial step places consecutive entries), its wave w the group's w-th.  False: the
// wave has no entry (a partial last workgroup, a shortened list) and returns.
template <int WAVES>
__device__ __forceinline__ bool list_wave_entry(int xcd_map, int n, int wave, int* entry) {
  const int groups = (n + WAVES - 1) / WAVES, g = (int)blockIdx.x;
  if (g >= groups) return false;
  const int i = (xcd_map ? xcd_board(g, groups) : g) * WAVES + wave;
  *entry = i;
  return i < n;
}

}  // namespace td
