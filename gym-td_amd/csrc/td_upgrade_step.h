// td_upgrade_step.h -- the enemy level of a summon as an integer test on the step count.
// Plain C++, no HIP: td_capi.hip calls it where a device constant block is built, and
// scripts/upgrade_step_host.cpp runs it alone (also under the host sanitizers).
//
// The reference summons a level-1 enemy when progress >= enemy_upgrade_at (TDBoard.py:201), with
// progress = steps / max_episode_steps (:301), an f64 quotient.  Correctly rounded division by a
// positive number is monotone in the dividend, so the set of step counts that pass is
// [upgrade_step, oo): the kernels test `steps >= upgrade_step` (summon_cluster, td_step_rules.h)
// and need no quotient of their own before a summon.
#pragma once
#include <cstdint>

namespace td {

// The smallest s in [0, 2^31 - 1] with (double)s / max_episode_steps >= enemy_upgrade_at:
// 0 for a threshold <= 0, INT32_MAX if there is none (a board's step counter is an int32 and
// cannot pass it).  max_episode_steps > 0 and a finite threshold: td_cfg_check.h.
inline int32_t upgrade_step(int32_t max_episode_steps, double enemy_upgrade_at) {
  const double m = (double)max_episode_steps;
  const int64_t top = INT32_MAX;
  if (enemy_upgrade_at <= 0.0) return 0;
  if ((double)top / m < enemy_upgrade_at) return INT32_MAX;
  // threshold * m is within a few units of the answer (two roundings); walk to it
  const double guess = enemy_upgrade_at * m;
  int64_t s = guess >= (double)top ? top : (int64_t)guess;
  while (s > 0 && (double)(s - 1) / m >= enemy_upgrade_at) --s;
  while (s < top && (double)s / m < enemy_upgrade_at) ++s;
  return (int32_t)s;
}

}  // namespace td
