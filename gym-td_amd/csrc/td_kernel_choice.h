// td_kernel_choice.h -- which step kernel TD_KERNEL_AUTO means, and when its observation
// stores are write-through, and the record a handle keeps of its choice (KernelChoice).  Plain
// C++, no HIP: functions of the handle's ints, which td_capi.hip calls (apply_kernel, the two
// kernel-kind setters, td_step) and scripts/kernel_choice_host.cpp and
// scripts/retained_kernel_host.cpp run alone, boundary by boundary and setter by setter.
// Kinds: 0 large, 1 small, 2 small2 (KernelChoice::small).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstdio>

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

// The kind of a skipping launch under TD_KERNEL_AUTO: a td_step into the retained buffer that
// leaves clean windows unwritten (StepArgs::obs_skip, td_obs_ledger.h).  full_kind is the kind
// of a launch that writes every window (auto_kernel_kind, or what td_set_step_kernel forced):
// that launch is bound by its stores, a skipping launch writes ~7.7 of 18.3 KB per board at
// 10x10 and is bound by the boards in flight -- so the second wave of small2, which halves
// them, has almost nothing left to write.  Returns full_kind wherever the sweep
// (scripts/retained_kernel_bench.py, three alternating 200-step blocks per kernel) shows no
// gain whose slowest block is below full_kind's fastest.  Every row was measured against
// both other kernels, so it holds whatever full_kind is.
// us per step, fastest-slowest of three blocks, profiles/retained_kernel/sweep.jsonl:
//   float32 L = 10 above one round of boards: the one-wave small kernel in every mode --
//     TD-def     12,288   small 41.8-42.3    small2 43.6-44.4    large 43.0-44.1
//                16,384         51.6-52.0           55.0-55.9          54.4-65.6
//                32,768         92.4-93.9           101.8-103.4        99.3-169.6
//                65,536         173.5-175.7         193.9-197.6        187.3-229.2
//     TD-atk     16,384         78.5-82.6           87.1-91.2          83.3-88.1
//                65,536         229.1-250.1         293.7-313.7        265.4-286.7
//     TD-2p      16,384         52.0-53.0           55.9-57.6          55.0-69.7
//                65,536         168.8-170.5         196.7-199.6        183.2-185.1
//     TD-def multi-action 16,384  61.0-61.6         64.3-64.8          67.1-81.6
//                65,536         191.0-193.0         217.7-218.9        221.1-221.6
//     TD-2p multi-action 16,384   61.7-62.2         65.4-66.1          66.8-71.6
//   L = 20 TD-2p multi-action 16,384: small2 189.2-191.0 vs 197.4-200.0 small, 197.5-200.3 large;
//   L = 30 TD-def 16,384: small2 278.0-281.1 vs 291.8-294.3 small, 292.9-294.9 large -- the full
//   kind stays: on the larger maps the second wave still pays.
//   The bench line (65,536 TD-def boards, burn-in 1,200): 439.0-440.3 vs 388.2-391.9 M env-steps/s,
//   148.9-149.3 vs 167.2-168.8 us per step, three alternating runs (bench_branch_*, bench_parent_*).
//   Up to one round of boards every board is in flight with any kernel: the full kind stays.
//   float16 at L = 10 runs the small kernel above half a round already (auto_kernel_kind).
inline int retained_kernel_kind(int L, int mode, int multi, int obs_fmt, int B, int resident, int resident2,
                                int full_kind) {
  (void)mode; (void)multi; (void)resident2;
  if (resident <= 0 || B <= resident) return full_kind;
  if (obs_fmt == TD_OBS_F32 && L == 10) return 1;
  return full_kind;
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

// What td_set_step_kernel and td_set_retained_step_kernel refuse of a kind (TD_KERNEL_AUTO ..
// TD_KERNEL_SMALL2) on a map side L.  fn: the caller's name, for the message.
inline bool kernel_kind_ok(const char* fn, int kind, int L, char* msg, size_t cap) {
  if (kind < TD_KERNEL_AUTO || kind > TD_KERNEL_SMALL2)
    std::snprintf(msg, cap, "%s: unknown kernel kind %d", fn, kind);
  else if (kind >= TD_KERNEL_SMALL && L != 10 && L != 20 && L != 30)
    std::snprintf(msg, cap, "%s: L = %d has no small-batch step kernel (only L = 10 / 20 / 30)", fn, L);
  else
    return true;
  return false;
}

// A handle's kernel choice, as one record (td_handle.kernel): both kinds of a handle.
// td_set_step_kernel forces both (a forced kind is forced for every launch),
// td_set_retained_step_kernel the second only; an unforced retained kind follows the rule on the
// full kind as resolved, forced or not.
struct KernelChoice {
  int small = 0, obs_wt = 0;  // the step kernel (0 large, 1 small, 2 small2), write-through observation stores
  int kernel_forced = 0;      // td_set_step_kernel chose the kind (else TD_KERNEL_AUTO: auto_kernel_kind)
  // A skipping launch (a td_step into the retained buffer with StepArgs::obs_skip) runs a kind
  // of its own (retained_kernel_kind): `small` stays the kind of a launch that writes every window.
  int small_retained = 0, obs_wt_retained = 0;
  int retained_forced = 0;    // td_set_step_kernel or td_set_retained_step_kernel chose small_retained
  int name_kind = 0;          // the kind td_step_kernel_name names: of the last td_step's launch, else `small`

  // td_set_step_kernel (kind as kernel_kind_ok passed it):
  // a forced kind is forced for every launch, skipping or not; TD_KERNEL_AUTO gives both back to their rules
  void force_both(int kind) {
    kernel_forced = retained_forced = kind != TD_KERNEL_AUTO;
    if (kind != TD_KERNEL_AUTO) small = small_retained = kind - 1;
  }
  // td_set_retained_step_kernel: skipping launches only.  TD_KERNEL_AUTO gives their kind back to
  // the rule (on the full kind as it stands, forced or not), any other kind forces it.  The kind
  // of a launch that writes every window stays.
  void force_retained(int kind) {
    retained_forced = kind != TD_KERNEL_AUTO;
    if (kind != TD_KERNEL_AUTO) small_retained = kind - 1;
  }
  // Both kinds, resolved: a forced kind stays as it stands, any other follows its rule above;
  // then whether each kind's observation stores are write-through.  The name goes back to the
  // kernel of a launch that writes every window.
  void resolve(int L, int mode, int multi, int obs_fmt, int B, int resident, int resident2) {
    if (!kernel_forced) small = auto_kernel_kind(L, mode, multi, obs_fmt, B, resident, resident2);
    if (!retained_forced) small_retained = retained_kernel_kind(L, mode, multi, obs_fmt, B, resident, resident2, small);
    obs_wt = obs_write_through(small, L, obs_fmt, B);
    obs_wt_retained = obs_write_through(small_retained, L, obs_fmt, B);
    name_kind = small;
  }
  // The kernel is chosen per launch: a launch that writes every window is bound by its stores,
  // a skipping launch by the boards in flight (retained_kernel_kind).
  int kind(int obs_skip) const { return obs_skip ? small_retained : small; }
  int write_through(int obs_skip) const { return obs_skip ? obs_wt_retained : obs_wt; }
};

}  // namespace td
