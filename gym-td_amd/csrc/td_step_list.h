// td_step_list.h -- the partial step of a device-resident list (td_step_boards_dev): the common
// body of the kernels in td_step_list.hip (float32 observation) and td_step_list_f16.hip.  The
// step itself is td_step_sel.h's step_sel_body, unchanged; in front of it the list's length is
// made of two words in device memory: the count (or cap, where the caller gave none) and the
// verdict of the check kernel launched in front (td_list_check.hip).  A refused list has
// length 0: every wave exits before it reads an id or anything of any board.
#pragma once
#include "td_step_sel.h"

namespace td {

// ids: [cap] device memory; count: [1] or nullptr; verdict: the handle's record.  Both words
// were written by earlier kernels on the stream and by no wave of this one, so they are read
// through the constant address space as step_sel_body reads its id: wave-uniform SMEM loads
// beside the argument loads, made visible by the kernel boundary.  The check kernel refused a
// count outside [0, cap], so n <= cap = the grid, and ids[0 .. n) were all range-checked.
template <int LT, int MODE, bool SCAN, class OT = float>
__device__ __forceinline__ void step_list_body(const StepArgs& a, const int32_t* ids, int cap, const int32_t* count,
                                               const td_list_status* verdict) {
  typedef __attribute__((address_space(4))) const int32_t cword_t;
  const int code = reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(verdict))[0];
  static_assert(offsetof(td_list_status, code) == 0, "the verdict's first word");
  int n = cap;
  if (count) n = reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(count))[0];
  n = code ? 0 : n;
  step_sel_body<LT, MODE, SCAN, OT>(a, ids, n);
}

}  // namespace td
