// td_list_check.hip -- td_list_check_kernel: the validation of a device-resident board list
// (td_step_boards_dev, td_copy_boards_dev), run on the step's stream in front of the kernel
// that consumes the list.  One thread per entry: the range test, one mark in the handle's
// scratch (td_list_check.h: an atomic max that returns the old word, so the second of two
// conflicting entries sees the conflict), and for an entry with a defect one atomic min into the
// call's key.  The block that arrives last (a ticket counter) makes the 16-byte verdict of the
// key, writes it where the consumer reads it and where the caller asked for it, counts a
// refusal, and leaves key and counter as the next call needs them.  Every word shared between
// blocks is touched by agent-scope atomics only; what the last block writes is read by later
// kernels only, behind the kernel boundary.
#include "td_kernels.h"

namespace td {

__global__ __launch_bounds__(kListCheckThreads) void td_list_check_kernel(ListCheckArgs a) {
  const int i = (int)(blockIdx.x * kListCheckThreads + threadIdx.x);
  const int n = a.count ? *a.count : a.cap;  // block-uniform; written before this kernel, never by it
  const bool bad_count = n < 0 || n > a.cap;
  unsigned long long key = kListNoDefect;
  if (bad_count) {
    if (i == 0) key = list_key(TD_LIST_BAD_COUNT, 0, 0);  // (no entry is read as an id)
  } else if (i < n) {
    const int d = a.dst[i];
    if (d < 0 || d >= a.B) {
      key = list_key(TD_LIST_RANGE, i, 1);
    } else {
      const uint32_t old = __hip_atomic_fetch_max(&a.marks[d], list_mark(a.epoch, kListDst), __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
      const int c = list_conflict(list_seen(old, a.epoch), kListDst);
      if (c != TD_LIST_OK) key = list_key(c, i, 1);
    }
    if (a.src) {
      const int s = a.src[i];
      // A fan-out names one source in every entry, and thousands of atomics on one word go one
      // after the other (4,095 children: 50 us of check in front of a 20-us copy,
      // profiles/board_lists_dev).  So the wave's first active lane marks its source for every
      // lane that names the same board, and hands them the old word: one atomic per wave there.
      const int s0 = __builtin_amdgcn_readfirstlane(s);
      const int first = __ffsll((unsigned long long)__ballot(1)) - 1;
      uint32_t old0 = 0;
      if (s0 >= 0 && s0 < a.B) {  // wave-uniform
        if ((int)(threadIdx.x & 63u) == first)
          old0 = __hip_atomic_fetch_max(&a.marks[s0], list_mark(a.epoch, kListSrc), __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
        old0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)old0);
      }
      unsigned long long k = kListNoDefect;
      if (s < 0 || s >= a.B) {
        k = list_key(TD_LIST_RANGE, i, 0);
      } else {
        const uint32_t old = s == s0 ? old0
                                     : __hip_atomic_fetch_max(&a.marks[s], list_mark(a.epoch, kListSrc), __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT);
        const int c = list_conflict(list_seen(old, a.epoch), kListSrc);
        if (c != TD_LIST_OK) k = list_key(c, i, 0);
      }
      key = k < key ? k : key;
    }
  }
  if (key != kListNoDefect) {
    // (the returning form, its result kept live: the wave waits for the atomic itself)
    const unsigned long long was = __hip_atomic_fetch_min(&a.st->key, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::"v"(was));
  }
  // every atomic of this block has been performed before its ticket is drawn
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x != 0) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uint32_t ticket = __hip_atomic_fetch_add(&a.st->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket != gridDim.x - 1) return;
  // ---- the last block: every other block's atomics are in the key
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long k = __hip_atomic_exchange(&a.st->key, kListNoDefect, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&a.st->arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  td_list_status v;
  v.code = list_key_code(k);
  v.call = a.call;
  v.entry = -1;
  v.board = -1;
  if (v.code == TD_LIST_BAD_COUNT) {
    v.board = n;
  } else if (v.code != TD_LIST_OK) {
    v.entry = list_key_entry(k);  // (< n <= cap: the entry was read above)
    v.board = (list_key_side(k) ? a.dst : a.src)[v.entry];
  }
  a.st->verdict = v;
  if (a.status) *a.status = v;
  if (v.code != TD_LIST_OK) {
    const uint32_t r = a.st->refused;  // (written by an earlier call's last block, or the host)
    a.st->refused = r + 1;
    if (r == 0) a.st->first = v;
  }
}

hipError_t launch_list_check(const ListCheckArgs& a, hipStream_t s) {
  const int blocks = (a.cap + kListCheckThreads - 1) / kListCheckThreads;
  hipLaunchKernelGGL(td_list_check_kernel, dim3(blocks), dim3(kListCheckThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace td
