// td_step_body.h -- the batched gym-TD step on CDNA4 (gfx950).
//
// One 64-lane wavefront (= one workgroup) owns one board for the whole step:
// the board's slice of the SoA record is staged in LDS, every serial phase of the
// reference runs wave-uniform with wave ballots standing in for the reference's
// "first enemy in list order" scans, and the (45, L, L) float32 observation is
// written with 16-byte coalesced stores straight from LDS tables.
//
// Reference order of one env step:
//   cool-downs                     TDDefense.py:38-39 / TDAttack.py:31-32 / TDMulti.py:50-51
//   defender action                TDDefense.py:40-77, TDMulti.py:208-258
//   attacker action / opponent     TDGymBasic.py:81-108, TDAttack.py:36-48, TDMulti.py:199-241
//   TDBoard.step                   TDBoard.py:295-368
//   done / get_states / info       TDBoard.py:370-385, 85-144, TDDefense.py:81-87
//
// Floating point: the file is compiled with -ffp-contract=off and every f64/f32
// operation is an explicit correctly-rounded intrinsic where the reference's
// Python/numpy rounding order matters.
//
// What belongs here: step_board, one board's whole step in the reference's order, built
// from the pieces of td_step_state.h, td_step_rules.h, td_step_opp.h and td_step_obs.h;
// the one-wave kernels' common body (step_kernel_body) and the occupancy attributes of the
// small-batch kernels.  The kernels themselves are in td_step.hip (float32 observation)
// and td_step_f16.hip (float16), the two-wave kernel's text in td_step_small2.inc.
#pragma once
#include "td_board.h"
#include "td_kernels.h"
#include "td_step_obs.h"
#include "td_step_opp.h"
#include "td_step_rules.h"
#include "td_step_state.h"
#include "td_wave.h"

namespace td {

// SCAN: the multi-action defender scan is compiled in (launched only when a.multi).
// Its 16-B staging buffers raise the 30x30 kernel from 55 to 148 VGPRs, and the
// discrete kernel should not pay for them in occupancy.
// SMALL: the batch runs as one round of waves (td_step_kernel_small); with a.obs_wt
// the observation lines are stored write-through (write_obs_lines).  (Storing the
// layout and tower planes at the start of the step, before the step logic, was
// measured slower at 4,096 and 8,192 boards: 36.3 / 53.1 vs 25.7 / 38.3 us.)

// SPLIT: the board's workgroup has a second wave (td_step_kernel_small2) that waits at
// the one workgroup barrier of this path and then writes the second half of the
// observation windows.
template <int NC, int LT, int MODE, bool SCAN, bool SMALL, bool SPLIT = false, class OT = float>
__device__ __forceinline__ void step_board(Smem<NC>& S, const Ctx& x, const StepArgs& a, int b, const Prefetch& P,
                                           StepOut* so = nullptr) {
  const TdDevCfg& C = x.C;
  uint32_t* const opp = a.opp_mt + (size_t)b * OPP_WORDS;
  uint32_t* const hot = a.opp_hot + (size_t)b * HOT_WORDS;
  U u;
  constexpr int PF = SMALL ? PF_SMALL : PF_LARGE;
  load_board<NC, PF, PF>(S, u, x, a, b, P);
  // what the dirty classes compare with after the step (obs_dirty), kept in LDS: the small
  // kernels have no SGPR to carry it across the step
  if (x.lane == 0) {
    S.before = cost_bits(u.cost_def, C);
    S.before_lp = u.base_LP;
  }
  const int64_t act_in =(int64_t)(((uint64_t)lane_word(P.w, PF_ACT + 1) << 32) | lane_word(P.w, PF_ACT));
  // built-in opponent stream: position, lazy-twist boundary and the next draws
  // (pre-computed by the previous step) come from the board's hot record
  WaveMt R{opp, lane_word(P.w, PF_HOT + 0), lane_word(P.w, PF_HOT + 1)};
  // The large kernel refills the pre-drawn outputs only when they run short (lazy); the
  // small kernels (no SGPR to spare at 8 waves per SIMD) refill every step and use a cache
  // only if it starts at the current position.
  constexpr bool LAZY_HOT = !SMALL;
  if constexpr (LAZY_HOT) {
    R.cn = lane_word(P.w, PF_HOT + 2);
    R.cbase = lane_word(P.w, PF_HOT + 3);
  } else {
    R.cn = lane_word(P.w, PF_HOT + 3) == R.pos ? lane_word(P.w, PF_HOT + 2) : 0u;
    R.cbase = R.pos;
  }
  R.cache = __shfl(P.w, PF_HOT + 4 + (x.lane < HOT_CACHE ? x.lane : 0));
  // (the early window in the large kernel too: +-0, reads +29 B per board, r04/s18)
  constexpr bool EARLY_MT = SMALL && !SCAN && MODE != MODE_2P;
  if constexpr (EARLY_MT) R.early_issue(x.lane);
  constexpr bool SCAN2 = SPLIT && SCAN;
  if (u.num_roads < 1 || u.num_roads > 3) {
    // never reset (its road generation failed): nothing to step
    const int nf = NCH * x.NCr;
    OT* o = reinterpret_cast<OT*>(a.obs) + (size_t)b * nf;
    for (int i = x.lane; i < nf; i += 64) o[i] = (OT)0.0f;
    if (x.lane == 0) {  // every output defined: done, no reward, no action taken
      a.hdr[b].flags = u.flags | FLAG_NO_LAYOUT;
      a.reward[b] = 0.0;
      a.done[b] = 1;
      if (a.win) a.win[b] = -1;
      if (a.allow_next) a.allow_next[b] = 0;
      if (a.cooldowns) a.cooldowns[b] = 0;
      if (a.fail_def) a.fail_def[b] = 0;
      if (a.real_def && !a.multi) a.real_def[b] = (int64_t)6 * x.NCr;
      if (a.ep_return) a.ep_return[b] = 0.0;
      if (a.ep_len) a.ep_len[b] = 0;
    }
    if (a.real_def && a.multi)
      for (int i = x.lane; i < 6 * x.NCr; i += 64) a.real_def[(size_t)b * 6 * x.NCr + i] = 0;
    if (a.fail_atk && x.lane < 3) a.fail_atk[(size_t)b * 3 + x.lane] = -1;
    if (a.real_atk && x.lane < 24) a.real_atk[(size_t)b * 24 + x.lane] = 4;
    if constexpr (SPLIT) {
      if (x.lane == 0) { S.early_go = 0u; so->go = 0u; }
      if constexpr (SCAN2) __syncthreads();  // (A0)
      __syncthreads();  // (A)
      __syncthreads();  // (B)
      __syncthreads();  // (C)
    }
    return;
  }
  OT* const obs = reinterpret_cast<OT*>(a.obs) + (size_t)b * NCH * x.NCr;
  const bool wt = a.obs_wt != 0;

  u.atk_cd = u.atk_cd - 1 > 0 ? u.atk_cd - 1 : 0;
  u.def_cd = u.def_cd - 1 > 0 ? u.def_cd - 1 : 0;
  const int64_t empty_def = (int64_t)6 * x.NCr;
  int fail_def = 0;
  int64_t real_def = empty_def;

  // ---- defender
  if (MODE != MODE_ATK) {
    if constexpr (SCAN2) {
      __syncthreads();  // (A0) the second wave has folded the flags
      defender_scan<NC, false, false>(S, u, x, nullptr, nullptr, u.def_cd == 0, so->scan_bad != 0u);
    } else if (SCAN) {
      defender_scan(S, u, x, a.def_act + (size_t)b * 6 * x.NCr,
                    a.real_def ? a.real_def + (size_t)b * 6 * x.NCr : nullptr, u.def_cd == 0);
    } else {
      int64_t act = act_in;
      if (act < 0 || act > empty_def) { u.flags |= FLAG_BAD_ACTION; act = empty_def; }
      if (u.def_cd == 0 && act != empty_def) {
        // op = act // L^2, row = (act // L) % L, column = act % L (TDDefense.py:65-67)
        const int a32 = (int)act, ncr = LT ? LT * LT : x.NCr;
        const int op = a32 / ncr;
        fail_def = defender_op(S, u, x, op, a32 - op * ncr);
        if (fail_def == FC_OK) { u.def_cd = C.def_interval; real_def = act; }
      }
    }
  }
  // ---- attacker
  if (MODE == MODE_DEF) {
    with_opp_rng(a, b, x.lane, R, [&](auto& G) { opponent_enemy(S, u, x, G, a.difficulty); });
  } else {
    attacker_actions<NC, MODE>(S, u, x, a, b);
    // info of the attacker now: its LDS arrays share space with the observation tables
    if (a.fail_atk && x.lane < 3) a.fail_atk[(size_t)b * 3 + x.lane] = S.fail_atk[x.lane];
    if (a.real_atk && x.lane < 24) a.real_atk[(size_t)b * 24 + x.lane] = S.real_atk[x.lane];
    if (MODE == MODE_ATK)
      with_opp_rng(a, b, x.lane, R, [&](auto& G) { opponent_tower(S, u, x, G, a.difficulty); });
  }
  // the towers and map[6] are final: cell words back to HBM if they changed, then
  // packed for the rest of the step (board_step reads the packed direction and distance)
  store_cells(S, u, x, a, b);
  u.cells_dirty = false;
  pack_obs_cells(S, x);
  // pre-draw the next step's words: loads issued now, consumed at the end of the step
  // (the step's draws are done: refill the pre-drawn outputs if the next step may run short)
  const bool refill = MODE != MODE_2P && (EARLY_MT || !LAZY_HOT || R.cached_left() < (uint32_t)HOT_REFILL);
  // (the multi-action kernels have no registers to carry the loads across the step: at once)
  if (refill && !EARLY_MT) {
    if constexpr (SCAN) R.prefetch(x.lane);
    else R.prefetch_issue(x.lane);
  }
  wsync();
  if constexpr (SPLIT) {  // (A): the second wave writes the binary-plane windows while this one steps
    // (its windows hold static and tower planes only: with the skip, the tower windows of a
    // board whose tower list changed -- a board that auto-resets rewrites every window below)
    if (x.lane == 0) S.early_go = kEarlyGo | (a.obs_skip ? (u.tw_dirty ? (uint32_t)OD_TOWER : 0u) : (uint32_t)OD_ALL);
    __syncthreads();
  }

  // ---- TDBoard.step
  // (parallel targeting: +1.1-1.4 % at 8,192 / 4,096 boards, -0.7 % in the large kernel at 65,536, profiles/r03/s29)
  double reward = board_step<NC, SMALL && !(SPLIT && LT == 20 && MODE == MODE_DEF && !SCAN)>(S, u, x, a, b);
  // The next step's opponent words, loaded since the attacker phase, are consumed here,
  // before this step's state stores: gfx950 counts loads and stores in one vmcnt, so
  // after the stores the wait for these loads became a wait for every store's
  // acknowledgement (s_waitcnt vmcnt(0)).  (Holding every state store back to the end
  // of the step, next to the observation, measured slower: 219 vs 216 us at 65,536
  // boards, 35.8 vs 34.9 at 8,192, profiles/r03/s16.)
  // (consumed here rather than before the board step: 8,192 boards 32.6-32.7 vs 33.2-33.3 us, r04/s13)
  if constexpr (EARLY_MT) {
    R.early_finish(x.lane);
  } else if (!SCAN && refill) R.prefetch_finish(x.lane);
  if (MODE == MODE_ATK) reward = -reward;                   // TDAttack.py:50
  const bool done = (u.base_LP <= 0) || (u.steps >= C.max_episode_steps);  // :384-385
  u.ep_ret = dadd(u.ep_ret, reward);
  const int ep_steps = u.steps;
  int8_t win = -1;
  if (done) {
    if (MODE == MODE_ATK) win = u.base_LP <= 0 ? 1 : 0;
    else win = u.base_LP > 0 ? 1 : 0;
  }
  // info['AllowNextMove'] (bits 0-1), and the env's attacker_cd / defender_cd attributes
  // after the step, saturated at 15 (td_step_io.cooldowns)
  const uint8_t allow = (uint8_t)((u.atk_cd <= 1 ? 1 : 0) | (u.def_cd <= 1 ? 2 : 0));
  const int acd = u.atk_cd < 15 ? u.atk_cd : 15, dcd = u.def_cd < 15 ? u.def_cd : 15;
  const uint8_t cool = (uint8_t)(acd | (dcd << 4));
  const double ep_ret = u.ep_ret;

  if (done) u.episodes += 1;
  bool was_reset = false;
  uint32_t lay_head = 0;
  if (done && a.autoreset && !a.opp_np) {  // random_agent=False: td_autoreset_kernel follows
    // consume staged layout number lay_head, published by a refill kernel on a side
    // stream while this grid may be running: relaxed sc1 poll of its tag, then one
    // agent-scope acquire before the plain vector loads of the record
    // (MI355X_MICROARCH.md § visibility, "Valid forms"; producer side: wave_layout)
    lay_head = a.lay_head[b];
    const uint32_t* rec = a.nxt + ((size_t)b * NSLOT + lay_head % NSLOT) * a.slot_words;
    const uint32_t want = slot_tag(lay_head);
    bool ready = ld_relaxed(rec) == want;
    // a dry ring: wait for the refill drawing this layout, or draw it now
    if (!ready) ready = take_dry_ring(a, b, lay_head, &u.flags);
    if (ready) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      reset_board(S, u, x, rec);
      was_reset = true;
    } else {
      u.flags |= FLAG_NO_LAYOUT;  // 65 failing draws in a row (the reference raises): the board keeps its finished episode
    }
  }
  // The enemy list back to HBM (after the layout poll's loads, whose wait would
  // otherwise wait for these stores too; a reset board has none).
  store_enemies(S, u, x, a, b);
  if constexpr (SPLIT) {
    // the new episode's layout first (the second wave stores the board next)
    if (was_reset) {
      store_cells(S, u, x, a, b);
      pack_obs_cells(S, x);
    }
  }
  if (x.lane == 0) {
    if (was_reset)  // the record has been read into LDS: its slot may be redrawn
      st_relaxed(a.lay_head + b, lay_head + 1u);
    sst(&hot[0], R.pos);
    sst(&hot[1], R.tw);
    sst(&hot[2], R.cn);
    sst(&hot[3], R.cbase);
  }
  if (refill && x.lane < HOT_CACHE) sst(&hot[4 + x.lane], R.cache);
  const uint32_t dirty = obs_dirty(S, u, C, a.obs_skip != 0, was_reset);
  // the channels the written windows read (both waves'): what channel_scalars must provide
  uint64_t need = kChAll;
  if constexpr (LT != 0) {
    if ((reinterpret_cast<uintptr_t>(a.obs) & (ObsFmt<OT>::UB - 1)) == 0) need = obs_need<LT, OT>(obs, dirty);
  }
  if constexpr (SPLIT) {
    // (B) the second wave's early pass has landed; it takes the board and the outputs
    // and stores them while this wave computes the statistics and broadcast channels;
    // (C) both are in LDS: each wave writes half of the windows the early pass left -- a
    // board that auto-reset this step has a new layout, and this wave rewrites every window.
    if (x.lane == 0) {  // field by field: no second register copy of the board
      so->hdr = hdr_of(u);
      so->nt = u.nt; so->tw_dirty = u.tw_dirty ? 1 : 0;
      so->reward = reward; so->ep_ret = ep_ret; so->real_def = real_def;
      so->ep_steps = ep_steps; so->fail_def = fail_def;
      so->done = done ? 1u : 0u; so->win = (uint32_t)(int32_t)win; so->allow = allow; so->cool = cool;
      so->go = was_reset ? 2u : 1u; so->any = u.n > 0 ? 1u : 0u; so->dirty = dirty;
      so->hdr_hi = (was_reset || done || u.flags != S.flags0) ? 1u : 0u;
    }
    __syncthreads();
    enemy_stats(S, u, x);  // no-op for a board without enemies (e.g. just reset)
    channel_scalars(S, u, x, need);
    __syncthreads();
    if (was_reset) write_obs_lines<NC, LT, 0, -1, 4, 0, OT>(S, x.lane, obs, u.n > 0, wt, a.edge_wt);
    // (every class dirty -- a step that may not skip: the writer without the skip's table reads
    // and tests, 203 vs 207 us at 65,536 boards, 32.0 vs 34.9 at 8,192; profiles/obs_retain/two_path_ab.log)
    else if (dirty == OD_ALL) write_obs_lines<NC, LT, 0, obs_late_half<LT, OT>(), 4, 2, OT>(S, x.lane, obs, u.n > 0, wt, a.edge_wt);
    else write_obs_lines<NC, LT, 0, obs_late_half<LT, OT>(), 4, 2, OT, true>(S, x.lane, obs, u.n > 0, wt, a.edge_wt, dirty);
  } else {
    enemy_stats(S, u, x);  // no-op for a board without enemies (e.g. just reset)
    channel_scalars(S, u, x, need);
    if (was_reset) {  // the new episode's layout
      store_cells(S, u, x, a, b);
      pack_obs_cells(S, x);
    }
    store_board(S, u, x, a, b, was_reset || done || u.flags != S.flags0);
    store_outputs(a, b, reward, ep_ret, real_def, ep_steps, fail_def, done, win, allow, cool, x.lane);
    // the observation last: nothing of the step is live any more, the writer has the registers
    if constexpr (LT != 0) {
      if ((reinterpret_cast<uintptr_t>(a.obs) & (ObsFmt<OT>::UB - 1)) == 0) {
        if (dirty == OD_ALL) write_obs_lines<NC, LT, 0, -1, 4, 0, OT>(S, x.lane, obs, u.n > 0, wt, a.edge_wt);
        else write_obs_lines<NC, LT, 0, -1, 4, 0, OT, true>(S, x.lane, obs, u.n > 0, wt, a.edge_wt, dirty);
      } else {
        write_obs<NC, LT, OT>(S, x, obs, u.n > 0);
      }
    } else {
      write_obs<NC, LT, OT>(S, x, obs, u.n > 0);
    }
  }
}

// One workgroup (one wave) per board.  (A persistent variant that prefetched the
// next board while stepping the current one measured slower: its static board
// assignment leaves a one-board tail, and the step is bound by HBM writes.)
// The kernel arguments a step needs before its board's loads go out, read together at the
// top: read where each is used they were six dependent scalar loads, each waited for, in
// front of every board's first load.
__device__ __forceinline__ void prologue_args(const StepArgs& a) {
  asm volatile("" ::"s"(a.B), "s"(a.xcd_map), "s"(a.multi), "s"(a.cfg), "s"(a.hdr), "s"(a.en_lp), "s"(a.en_mg),
               "s"(a.en_inf), "s"(a.tw_cd), "s"(a.tw_inf), "s"(a.cells), "s"(a.opp_hot), "s"(a.def_act));
}

template <int LT, int MODE, bool SCAN, bool SMALL, class OT = float>
__device__ __forceinline__ void step_kernel_body(const StepArgs& a) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ Smem<NC> S;
  const int i = (int)blockIdx.x;
  prologue_args(a);
  if (i >= a.B) return;
  const int b = a.xcd_map ? xcd_board(i, a.B) : i;
  const int L = LT ? LT : a.L;
  const Ctx x{S.cfg, L, L * L, (int)(threadIdx.x & 63), a.cfgs, a.epoch};
  const uint4 cfgv = load_cfg(a.cfg, x.lane);
  Prefetch P;
  constexpr int PF = SMALL ? PF_SMALL : PF_LARGE;
  prefetch_issue<PF, PF>(P, a, b, x.lane, x.NCr, MODE != MODE_ATK && !a.multi);
  store_cfg(S, cfgv, x.lane);  // (its load issued first: this wait leaves the board's loads in flight)
  wsync();  // every lane reads the block: no LDS access may move above its store
  step_board<NC, LT, MODE, SCAN, SMALL, false, OT>(S, x, a, b, P);
}

// The two-wave 20x20 TD-atk kernel does not fit 64 VGPRs: at 8 waves per SIMD it spilled
// (8 B of scratch per lane), so 6.  (The multi-action scan kernels ran at 5 until the
// flag fold's loop was kept rolled, scan_fold.)  Nor does any two-wave 20x20 kernel with the
// float16 observation (61-64 VGPRs in float32, 20 B of scratch per lane in float16 at 8): 6.
template <int LT, int MODE, bool SCAN, class OT = float>
constexpr int small2_cap() { return LT == 20 && ((MODE == MODE_ATK && !SCAN) || sizeof(OT) == 2) ? 6 : 8; }
#define TD_SMALL_ATTR __attribute__((amdgpu_waves_per_eu(8, 8)))
// (TD_SMALL2_OT: the output element of the kernel being stamped out, td_step_small2.inc)
#define TD_SMALL2_ATTR \
  __attribute__((amdgpu_waves_per_eu(small2_cap<LT, MODE, SCAN, TD_SMALL2_OT>(), small2_cap<LT, MODE, SCAN, TD_SMALL2_OT>())))

}  // namespace td
