// td_mask.h -- what the next step would answer to one action, decided from the board's
// present state: the comparisons tower_build / tower_lvup / tower_destruct / summon_cluster
// make (td_step_rules.h), in their order, without the step's side effects.  Shared by the mask
// kernel (td_mask.hip) and any host code that wants the same verdicts.
#pragma once
#include "td_board.h"
#include "td_common.h"

namespace td {

// tower_build (TDBoard.py:226-247) + the device's tower capacity: cost, position, capacity
__host__ __device__ inline int mask_build_code(double cost_def, double price, uint32_t cellw, int n_tw) {
  if (cost_def < price) return FC_COST;
  if (cw_block(cellw) > 0) return FC_POS;
  if (n_tw >= TCAP) return FC_CAP;
  return FC_OK;
}

// tower_lvup (:249-271) of the tower `ti` standing on the cell (has = false: none there)
__host__ __device__ inline int mask_lvup_code(bool has, uint32_t ti, double cost_def, const TdDevCfg& C) {
  if (!has) return FC_TARGET;
  const int lv = tw_lv(ti);
  if (lv >= C.max_tower_lv) return FC_LVMAX;
  if (cost_def < C.t_price[tw_type(ti)][lv + 1]) return FC_COST;
  return FC_OK;
}

// tower_destruct (:273-293)
__host__ __device__ inline int mask_destruct_code(bool has) { return has ? FC_OK : FC_TARGET; }

// The header of a board that was reset (a board whose road generation failed is not stepped).
__host__ __device__ inline bool mask_board_live(int num_roads) { return num_roads >= 1 && num_roads <= 3; }

// The cool-down gate after the step's decrement (TDDefense.py:38-39,64; TDAttack.py:31-33).
__host__ __device__ inline bool mask_cd_open(int cd) { return cd <= 1; }

// Enemy level of a summon in the next step: progress as the header's steps give it
// (TDBoard.py:201; IEEE division, as the step's ddiv).
__host__ __device__ inline int mask_enemy_lv(int steps, const TdDevCfg& C) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double progress = __ddiv_rn((double)steps, (double)C.max_episode_steps);
#else
  const double progress = (double)steps / (double)C.max_episode_steps;
#endif
  return progress >= C.enemy_upgrade_at ? 1 : 0;
}

// One enemy of type t (< 4) as the first of a cluster on `road` (summon_cluster, :199-224)
__host__ __device__ inline bool mask_summon_ok(int road, int t, int lv, int num_roads, int atk_cd, int n_en, double cost_atk,
                                               const TdDevCfg& C) {
  return mask_board_live(num_roads) && road < num_roads && mask_cd_open(atk_cd) && n_en < ECAP &&
         !(cost_atk < C.e_cost[t][lv]);
}

// One byte per action while a board's row is put together (td_mask.hip): the fail code in
// the low nibble, and two marks the outputs are derived with --
//   code byte = b & 0x0f;   mask byte = (b == 0 && the side may act) || (b & kMaskAlways)
constexpr uint32_t kMaskAlways = 0x20u;  // the no-op: code 0, always legal
constexpr uint32_t kMaskPad = 0x10u;     // padding inside the pitch: code 0, mask 0
// four bytes at once (every byte < 0x80, so the add carries into no neighbour)
__host__ __device__ inline uint32_t mask_code4(uint32_t x) { return x & 0x0f0f0f0fu; }
__host__ __device__ inline uint32_t mask_legal4(uint32_t x, bool open) {
  const uint32_t zero = (~(x + 0x7f7f7f7fu) >> 7) & 0x01010101u;
  return (open ? zero : 0u) | ((x >> 5) & 0x01010101u);
}

}  // namespace td
