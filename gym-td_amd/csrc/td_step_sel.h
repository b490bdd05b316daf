// td_step_sel.h -- the partial step (td_step_boards): one wave per NAMED board, the boards
// taken from a list.  What belongs here: the kernels' common body (step_sel_body: the large
// kernel's body, td_step_body.h step_kernel_body with SMALL = false, with the board read from
// the list); device text only, the launch is td_step_launch.h's.  The kernels themselves are in
// td_step_sel.hip (float32 observation) and td_step_sel_f16.hip.
//
// Nothing of a board that is not in the list is read or written: every access of step_board is
// indexed by the board it is given, the observation writers store a board's own bytes of the
// two lines it shares with its neighbours, and the episode statistics are accumulated per board.
#pragma once
#include "td_step_body.h"

namespace td {

// ids: [n] board ids in device memory (validated on the host: every id in [0, a.B), none twice).
template <int LT, int MODE, bool SCAN, class OT = float>
__device__ __forceinline__ void step_sel_body(const StepArgs& a, const int32_t* ids, int n) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ Smem<NC> S;
  const int i = (int)blockIdx.x;
  prologue_args(a);
  asm volatile("" ::"s"(ids), "s"(n));
  if (i >= n) return;
  // consecutive list entries on one XCD, as the copy places consecutive pairs: a sorted run of
  // neighbouring boards shares that XCD's L2.  The id is read through the constant address
  // space (the list is written before the launch and by no kernel): a wave-uniform SMEM load
  // beside the argument reads above, waited for with them (lgkmcnt) where the board's loads
  // need it, while the constant block's load below is already in flight.  (As a plain load it
  // was a vector load waited for with vmcnt(0) in front of every other load of the wave:
  // 1.10x the large kernel at 65,536 boards of 10x10, profiles/step_boards.)
  typedef __attribute__((address_space(4))) const int32_t cid_t;
  const int b = reinterpret_cast<cid_t*>(reinterpret_cast<uintptr_t>(ids))[a.xcd_map ? xcd_board(i, n) : i];
  const int L = LT ? LT : a.L;
  const Ctx x{S.cfg, L, L * L, (int)(threadIdx.x & 63), a.cfgs, a.epoch};
  const uint4 cfgv = load_cfg(a.cfg, x.lane);
  Prefetch P;
  prefetch_issue<PF_LARGE, PF_LARGE>(P, a, b, x.lane, x.NCr, MODE != MODE_ATK && !a.multi);
  store_cfg(S, cfgv, x.lane);  // (its load issued first: this wait leaves the board's loads in flight)
  wsync();  // every lane reads the block: no LDS access may move above its store
  step_board<NC, LT, MODE, SCAN, false, false, OT>(S, x, a, b, P);
}

}  // namespace td
