// td_step_list.h -- the partial step of a device-resident list (td_step_boards_dev): the common
// body of the kernels in td_step_list.hip (float32 observation) and td_step_list_f16.hip.  The
// step itself is td_step_sel.h's step_sel_body, unchanged; in front of it the list's length is
// made of two words in device memory: the count (or cap, where the caller gave none) and the
// verdict of the check kernel launched in front (td_list_check.hip).  A refused list has
// length 0: every wave exits before it reads an id or anything of any board.
#pragma once
#include "td_list_dev.h"
#include "td_step_sel.h"

namespace td {

// ids: [cap] device memory; count: [1] or nullptr; verdict: the handle's record.  The length
// is td_list_dev.h's dev_list_length, read as step_sel_body reads its id; n <= cap = the grid,
// and ids[0 .. n) were all range-checked.
template <int LT, int MODE, bool SCAN, class OT = float>
__device__ __forceinline__ void step_list_body(const StepArgs& a, const int32_t* ids, int cap, const int32_t* count,
                                               const td_list_status* verdict) {
  step_sel_body<LT, MODE, SCAN, OT>(a, ids, dev_list_length(cap, count, verdict));
}

}  // namespace td
