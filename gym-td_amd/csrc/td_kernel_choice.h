// td_kernel_choice.h -- which step kernel TD_KERNEL_AUTO means, and when its observation
// stores are write-through.  Plain C++, no HIP: functions of the handle's ints, which
// td_capi.hip calls (auto_kernel, apply_kernel) and scripts/kernel_choice_host.cpp runs
// alone, boundary by boundary.  Kinds: 0 large, 1 small, 2 small2 (td_handle.small).
#pragma once
#include <stdint.h>

#include "../../include/tdstep.h"
#include "td_common.h"

namespace td {

// TD_KERNEL_AUTO: the small-batch kernel where the whole batch is one round of waves,
// two waves per board up to half a round -- and again over a few rounds, where the
// second wave's half of the observation shortens every board's step more than the
// halved residency costs (single-action boards, profiles/r03/s7, same box: 10x10
// 12,288 / 16,384 boards 237.8 / 255.4 vs 224.0 / 238.5 M env-steps/s with the large
// kernel, 32,768 a tie; 30x30 16,384 / 32,768 boards 30.8 / 31.9 vs 29.8 / 31.2 M, 65,536
// 30.0 vs 30.2 M; TD-2p 20x20 multi-action at 16,384: 48.0 vs 51.5 M in round 3, 54.0 vs
// 52.1 M on the round-4 build, r04/s10).
// td_set_step_kernel overrides.
// resident, resident2: boards resident at once with one wave and with two waves per board
// (step_resident_boards), for the format given.
inline int auto_kernel_kind(int L, int mode, int multi, int obs_fmt, int B, int resident, int resident2) {
  const bool f16 = obs_fmt == TD_OBS_F16;
  // two-wave kernel up to this many rounds (TD-2p 20x20 multi-action at 16,384 boards:
  // 303.3-303.6 vs 314-315 us per step with the large kernel, profiles/r04/s10; TD-def
  // 10x10 at every batch above one round since round 5: 32,768 / 49,152 / 65,536 boards
  // 107.5-107.9 / 156.5-156.8 / 203.4-204.1 vs 111.7-111.9 / 160.6-160.9 / 208.2-208.4 us,
  // profiles/r05/s33, s34)
  const int rounds2 = multi ? (L == 20 && mode == TD_MODE_2P ? 8 : 0)
                            : L == 10 ? (mode == TD_MODE_DEF ? (1 << 20) : 3) : L == 30 ? 10 : 0;
  // The float16 observation at 10x10: the one-wave small kernel at every batch above half a
  // round.  With half the bytes to store the step is bound by the boards in flight, not by
  // the store stream, and the second wave halves them (TD-def 12,288 / 16,384 / 32,768 /
  // 65,536 boards: 38.9 / 47.5 / 82.7 / 158.4 us per step against 45.2 / 57.1 / 103.4 /
  // 201.1 two-wave and 39.3 / 49.2 / 88.8 / 172.0 large; TD-atk at 16,384 and TD-2p at
  // 32,768 alike, profiles/obs_f16/f16_sizes.jsonl).  At 20x20 and 30x30 the three kernels
  // are within 1-3 % of each other in float16, the float32 rule's choice never the slowest.
  if (f16 && L == 10) return B <= resident2 ? 2 : 1;
  return B <= resident2                               ? 2
         : B <= resident                              ? 1
         : (int64_t)B <= (int64_t)rounds2 * resident  ? 2
                                                      : 0;
}

// Write-through observation stores go with the small kernels where the batch's observation
// fits the 256-MiB Infinity Cache (scripts/storepol.hip: 21.8 vs 30.0 us at 8,192 boards).
// (Write-through beyond the Infinity Cache -- any kernel, TD_OBS_WT=1 -- measured 1.5-1.7x
// slower steps at 16,384-65,536 boards, profiles/r03/s21.)
inline int obs_write_through(int kind, int L, int obs_fmt, int B) {
  const bool f16 = obs_fmt == TD_OBS_F16;
  const double obs_bytes = (double)B * NCH * (L * L) * (f16 ? 2.0 : 4.0);
  return kind && obs_bytes <= 192.0 * 1024 * 1024 ? 1 : 0;
}

}  // namespace td
