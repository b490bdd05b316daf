// td_cfg_check.h -- the host-side check of a td_config, before td_create / td_set_config copy
// it into a device constant block.  Plain C++, no HIP: td_capi.hip calls it before anything is
// allocated or changed, and scripts/cfg_check_host.cpp runs it alone under the address and
// undefined-behaviour sanitizers.
//
// td_config carries every number as a double, and the reference computes with whatever Python
// value paramConfig was given.  The device keeps five of them as int32 (td_common.h TdDevCfg:
// frozen_time, base_LP, tower_distance and the two action intervals), so a value that is not an
// integer cannot be represented: it is refused here, not truncated (the reference slows an
// enemy frozen with frozen_time = 2.5 for three marches, a truncated 2 for two).  A NaN or an
// infinity in any field is refused too: every range test below is false for a NaN, and a
// double -> int32 conversion of one is undefined.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>

#include "../../include/tdstep.h"

namespace td {

enum : int {
  CFG_OK = 0,
  CFG_TYPES,       // enemy_types / tower_types other than 4
  CFG_LEVELS,      // max_enemy_lv other than 1, max_tower_lv outside {0, 1}
  CFG_HYPER,       // max_cluster_length other than 8, max_num_of_roads other than 3
  CFG_EPISODE,     // max_episode_steps <= 0
  CFG_NOT_FINITE,  // a NaN or an infinity in a double field
  CFG_NOT_INT,     // a fraction in a field the device keeps as an integer
  CFG_RANGE,       // tower_distance, frozen_time, base_LP or an interval outside its range
  CFG_ENEMY_LP,    // an enemy_LP <= 0 (LP / maxLP in the observation)
};

// The bounds of the integer-valued fields: the diamond of td_step_rules.h (15), the 8-bit
// slowdown of an enemy word (255), the int32 header fields.
constexpr double kCfgMaxTowerDistance = 15, kCfgMaxFrozenTime = 255, kCfgMaxInt = 2147483647.0;

// msg is written on a refusal only.
inline int cfg_check(const td_config& c, char* msg, size_t cap) {
  if (c.enemy_types != 4 || c.tower_types != 4) {
    std::snprintf(msg, cap, "enemy_types / tower_types must be 4 (obs has 45 channels)");
    return CFG_TYPES;
  }
  if (c.max_enemy_lv != 1 || c.max_tower_lv < 0 || c.max_tower_lv > 1) {
    std::snprintf(msg, cap, "max_enemy_lv must be 1, max_tower_lv 0 or 1");
    return CFG_LEVELS;
  }
  if (c.max_cluster_length != 8 || c.max_num_of_roads != 3) {
    std::snprintf(msg, cap, "max_cluster_length must be 8, max_num_of_roads 3");
    return CFG_HYPER;
  }
  if (c.max_episode_steps <= 0) {
    std::snprintf(msg, cap, "max_episode_steps must be > 0");
    return CFG_EPISODE;
  }
  struct Field { const char* name; const double* v; int n; };
  const Field all[] = {
      {"enemy_LP", &c.enemy_LP[0][0], 8}, {"enemy_speed", &c.enemy_speed[0][0], 8},
      {"enemy_defense", &c.enemy_defense[0][0], 8}, {"enemy_cost", &c.enemy_cost[0][0], 8},
      {"tower_attack", &c.tower_attack[0][0], 8}, {"tower_range", &c.tower_range[0][0], 8},
      {"tower_splash_range", &c.tower_splash_range[0][0], 8}, {"tower_cost", &c.tower_cost[0][0], 8},
      {"tower_attack_interval", &c.tower_attack_interval[0][0], 8},
      {"tower_destruct_return", &c.tower_destruct_return, 1}, {"frozen_time", &c.frozen_time, 1},
      {"frozen_ratio", &c.frozen_ratio, 1}, {"attacker_init_cost", &c.attacker_init_cost, 1},
      {"defender_init_cost", &c.defender_init_cost, 1}, {"base_LP", &c.base_LP, 1}, {"max_cost", &c.max_cost, 1},
      {"reward_kill", &c.reward_kill, 1}, {"penalty_leak", &c.penalty_leak, 1}, {"reward_time", &c.reward_time, 1},
      {"attacker_cost_init_rate", &c.attacker_cost_init_rate, 1},
      {"attacker_cost_final_rate", &c.attacker_cost_final_rate, 1}, {"defender_cost_rate", &c.defender_cost_rate, 1},
      {"tower_distance", &c.tower_distance, 1}, {"enemy_upgrade_at", &c.enemy_upgrade_at, 1},
      {"attacker_action_interval", &c.attacker_action_interval, 1},
      {"defender_action_interval", &c.defender_action_interval, 1}};
  for (const Field& f : all)
    for (int i = 0; i < f.n; ++i)
      if (!std::isfinite(f.v[i])) {
        if (f.n > 1) std::snprintf(msg, cap, "%s[%d][%d] is not a finite number", f.name, i / 2, i % 2);
        else std::snprintf(msg, cap, "%s is not a finite number", f.name);
        return CFG_NOT_FINITE;
      }
  const Field ints[] = {{"frozen_time", &c.frozen_time, 1}, {"base_LP", &c.base_LP, 1},
                        {"tower_distance", &c.tower_distance, 1},
                        {"attacker_action_interval", &c.attacker_action_interval, 1},
                        {"defender_action_interval", &c.defender_action_interval, 1}};
  for (const Field& f : ints)
    if (*f.v != std::floor(*f.v)) {
      std::snprintf(msg, cap, "%s = %.17g is not an integer (the device keeps it as an int32)", f.name, *f.v);
      return CFG_NOT_INT;
    }
  if (c.tower_distance < 0 || c.tower_distance > kCfgMaxTowerDistance) {
    std::snprintf(msg, cap, "tower_distance out of range [0, 15]");
    return CFG_RANGE;
  }
  if (c.frozen_time < 0 || c.frozen_time > kCfgMaxFrozenTime) {
    std::snprintf(msg, cap, "frozen_time must be in [0, 255] (8-bit slowdown)");
    return CFG_RANGE;
  }
  if (c.base_LP < 1 || c.base_LP > kCfgMaxInt) {
    std::snprintf(msg, cap, "base_LP must be a positive int (None is not supported)");
    return CFG_RANGE;
  }
  if (c.attacker_action_interval < 0 || c.attacker_action_interval > kCfgMaxInt || c.defender_action_interval < 0 ||
      c.defender_action_interval > kCfgMaxInt) {
    std::snprintf(msg, cap, "attacker_action_interval / defender_action_interval must be in [0, 2^31 - 1]");
    return CFG_RANGE;
  }
  for (int t = 0; t < 4; ++t)
    for (int l = 0; l < 2; ++l)
      if (c.enemy_LP[t][l] <= 0) {
        std::snprintf(msg, cap, "enemy_LP must be > 0");
        return CFG_ENEMY_LP;
      }
  return CFG_OK;
}

}  // namespace td
