// td_step_skip.h -- frame skip (td_set_frame_skip): k board steps of every board in ONE
// launch, one observation written.  The board is loaded once, the sub-steps run on its LDS
// image in the reference's order (step_board's order, td_step_body.h), and the state, the
// step's outputs, the opponent's hot record and the observation are stored once, after the
// last sub-step the board ran.
//
//   sub-step 0         the caller's action (def_act / atk_act), as a step takes it
//   sub-steps 1..k-1   the empty action for every side the caller controls: the defender's
//                      6 L^2 and the attacker's all-4 clusters change nothing but the
//                      cool-downs, so the action phases are simply not run
//   built-in opponent  acts in every sub-step on the board's own stream, as in k steps
//   episode end        the board stops after the sub-step that finished its episode; with
//                      auto-reset its new episode starts there (one layout per launch)
//
// Between sub-steps nothing goes to HBM but what the rules need: the opponent's MT words
// once its pre-drawn outputs run short (WaveMt's slow path and pre-draw, with the large
// kernel's refill rule per sub-step, so the stream's words, position and lazy-twist
// boundary are those of k launches of td_step_kernel) and captured config blocks.
//
// What belongs here: skip_board (one board's macro step) and the kernels' common body,
// instantiated per observation format by td_step_skip.hip and td_step_skip_f16.hip (device
// text only: the launch is td_step_launch.h's).  The existing step kernels share no text with
// this path beyond the pieces it calls (board_step, defender_op, attacker_actions,
// opponent_*, enemy_stats, channel_scalars, reset_board, take_dry_ring, obs_dirty, the
// observation writers): step_board is untouched.
#pragma once
#include "td_step_body.h"

namespace td {

// TD-atk: the built-in defender builds and destroys towers in any sub-step, on the raw cell
// words (map[6] in bits 24-31, which the packed form pack_obs_cells leaves for board_step
// overwrites with the distance).  The raw words are kept beside the packed ones and swapped
// in for the sub-steps in which the opponent may act (its cool-down is 0).
template <int NC>
__device__ __forceinline__ void skip_copy_cells(uint32_t* dst, const uint32_t* src, int ncr, int lane) {
  for (int i = lane; i < ncr; i += 64) dst[i] = src[i];
  wsync();
}

template <int NC, int LT, int MODE, class OT>
__device__ __forceinline__ void skip_board(Smem<NC>& S, uint32_t* raw, const Ctx& x, const StepArgs& a, int b,
                                           const Prefetch& P) {
  const TdDevCfg& C = x.C;
  uint32_t* const opp = a.opp_mt + (size_t)b * OPP_WORDS;
  uint32_t* const hot = a.opp_hot + (size_t)b * HOT_WORDS;
  U u;
  load_board<NC, PF_LARGE, PF_LARGE>(S, u, x, a, b, P);
  // what the buffer holds: the board as loaded at the start of the macro step (obs_dirty)
  if (x.lane == 0) {
    S.before = cost_bits(u.cost_def, C);
    S.before_lp = u.base_LP;
  }
  const int64_t act_in = (int64_t)(((uint64_t)lane_word(P.w, PF_ACT + 1) << 32) | lane_word(P.w, PF_ACT));
  WaveMt R{opp, lane_word(P.w, PF_HOT + 0), lane_word(P.w, PF_HOT + 1)};
  R.cn = lane_word(P.w, PF_HOT + 2);
  R.cbase = lane_word(P.w, PF_HOT + 3);
  R.cache = __shfl(P.w, PF_HOT + 4 + (x.lane < HOT_CACHE ? x.lane : 0));
  const int64_t empty_def = (int64_t)6 * x.NCr;
  if (u.num_roads < 1 || u.num_roads > 3) {
    // never reset (its road generation failed): nothing to step, every output defined
    const int nf = NCH * x.NCr;
    OT* o = reinterpret_cast<OT*>(a.obs) + (size_t)b * nf;
    for (int i = x.lane; i < nf; i += 64) o[i] = (OT)0.0f;
    if (x.lane == 0) {
      a.hdr[b].flags = u.flags | FLAG_NO_LAYOUT;
      a.reward[b] = 0.0;
      a.done[b] = 1;
      if (a.win) a.win[b] = -1;
      if (a.allow_next) a.allow_next[b] = 0;
      if (a.cooldowns) a.cooldowns[b] = 0;
      if (a.fail_def) a.fail_def[b] = 0;
      if (a.real_def) a.real_def[b] = empty_def;
      if (a.ep_return) a.ep_return[b] = 0.0;
      if (a.ep_len) a.ep_len[b] = 0;
    }
    if (a.fail_atk && x.lane < 3) a.fail_atk[(size_t)b * 3 + x.lane] = -1;
    if (a.real_atk && x.lane < 24) a.real_atk[(size_t)b * 24 + x.lane] = 4;
    return;
  }
  OT* const obs = reinterpret_cast<OT*>(a.obs) + (size_t)b * NCH * x.NCr;
  const bool wt = a.obs_wt != 0;

  int fail_def = 0;
  int64_t real_def = empty_def;
  double total = 0.0;
  bool done = false, refilled = false;
  const int k = a.frame_skip;
#pragma unroll 1
  for (int j = 0; j < k; ++j) {
    u.atk_cd = u.atk_cd - 1 > 0 ? u.atk_cd - 1 : 0;
    u.def_cd = u.def_cd - 1 > 0 ? u.def_cd - 1 : 0;
    // the cell words are raw in sub-step 0 (as loaded); later only TD-atk needs them raw,
    // and only when its built-in defender is off cool-down (opponent_tower returns at once
    // otherwise, without a draw)
    const bool raw_cells = j == 0 || (MODE == MODE_ATK && u.def_cd == 0);
    if (MODE == MODE_ATK && j > 0 && raw_cells) skip_copy_cells<NC>(S.cell, raw, x.NCr, x.lane);
    if (j == 0) {
      // ---- the caller's action (sub-step 0 only)
      if (MODE != MODE_ATK) {
        int64_t act = act_in;
        if (act < 0 || act > empty_def) { u.flags |= FLAG_BAD_ACTION; act = empty_def; }
        if (u.def_cd == 0 && act != empty_def) {
          const int a32 = (int)act, ncr = LT ? LT * LT : x.NCr;
          const int op = a32 / ncr;
          fail_def = defender_op(S, u, x, op, a32 - op * ncr);
          if (fail_def == FC_OK) { u.def_cd = C.def_interval; real_def = act; }
        }
      }
      if (MODE != MODE_DEF) {
        attacker_actions<NC, MODE>(S, u, x, a, b);
        if (a.fail_atk && x.lane < 3) a.fail_atk[(size_t)b * 3 + x.lane] = S.fail_atk[x.lane];
        if (a.real_atk && x.lane < 24) a.real_atk[(size_t)b * 24 + x.lane] = S.real_atk[x.lane];
      }
    }
    // ---- the built-in opponent (every sub-step)
    if (MODE == MODE_DEF) with_opp_rng(a, b, x.lane, R, [&](auto& G) { opponent_enemy(S, u, x, G, a.difficulty); });
    if (MODE == MODE_ATK && raw_cells)
      with_opp_rng(a, b, x.lane, R, [&](auto& G) { opponent_tower(S, u, x, G, a.difficulty); });
    // the towers and map[6] are final for this sub-step: the raw cell words aside (TD-atk)
    // or back to HBM (sub-step 0 of the other modes, whose cells change there only), then
    // packed for board_step
    if (raw_cells) {
      if (MODE == MODE_ATK) {
        skip_copy_cells<NC>(raw, S.cell, x.NCr, x.lane);
      } else {
        store_cells(S, u, x, a, b);
        u.cells_dirty = false;
      }
      pack_obs_cells(S, x);
    }
    // pre-draw the opponent's next words if the next sub-step (or step) may run short:
    // the large kernel's rule, per sub-step
    const bool refill = MODE != MODE_2P && R.cached_left() < (uint32_t)HOT_REFILL;
    if (refill) { R.prefetch_issue(x.lane); refilled = true; }
    wsync();

    // ---- TDBoard.step
    double reward = board_step<NC, false>(S, u, x, a, b);
    if (refill) R.prefetch_finish(x.lane);
    if (MODE == MODE_ATK) reward = -reward;
    done = (u.base_LP <= 0) || (u.steps >= C.max_episode_steps);
    u.ep_ret = dadd(u.ep_ret, reward);
    total = j == 0 ? reward : dadd(total, reward);  // r0, then left to right
    if (done) break;
  }

  // ---- what the last executed sub-step would have written
  const int ep_steps = u.steps;
  int8_t win = -1;
  if (done) {
    if (MODE == MODE_ATK) win = u.base_LP <= 0 ? 1 : 0;
    else win = u.base_LP > 0 ? 1 : 0;
  }
  const uint8_t allow = (uint8_t)((u.atk_cd <= 1 ? 1 : 0) | (u.def_cd <= 1 ? 2 : 0));
  const int acd = u.atk_cd < 15 ? u.atk_cd : 15, dcd = u.def_cd < 15 ? u.def_cd : 15;
  const uint8_t cool = (uint8_t)(acd | (dcd << 4));
  const double ep_ret = u.ep_ret;

  if (done) u.episodes += 1;
  bool was_reset = false;
  uint32_t lay_head = 0;
  if (done && a.autoreset && !a.opp_np) {
    // consume staged layout number lay_head (step_board: relaxed poll of its tag, one
    // agent-scope acquire before the plain loads of the record) -- at most one per launch
    lay_head = a.lay_head[b];
    const uint32_t* rec = a.nxt + ((size_t)b * NSLOT + lay_head % NSLOT) * a.slot_words;
    const uint32_t want = slot_tag(lay_head);
    bool ready = ld_relaxed(rec) == want;
    if (!ready) ready = take_dry_ring(a, b, lay_head, &u.flags);
    if (ready) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      reset_board(S, u, x, rec);
      was_reset = true;
    } else {
      u.flags |= FLAG_NO_LAYOUT;
    }
  }
  store_enemies(S, u, x, a, b);
  if (x.lane == 0) {
    if (was_reset) st_relaxed(a.lay_head + b, lay_head + 1u);
    sst(&hot[0], R.pos);
    sst(&hot[1], R.tw);
    sst(&hot[2], R.cn);
    sst(&hot[3], R.cbase);
  }
  if (refilled && x.lane < HOT_CACHE) sst(&hot[4 + x.lane], R.cache);
  const uint32_t dirty = obs_dirty(S, u, C, a.obs_skip != 0, was_reset);
  uint64_t need = kChAll;  // the channels the written windows read (step_board)
  if constexpr (LT != 0) {
    if ((reinterpret_cast<uintptr_t>(a.obs) & (ObsFmt<OT>::UB - 1)) == 0) need = obs_need<LT, OT>(obs, dirty);
  }
  enemy_stats(S, u, x);
  channel_scalars(S, u, x, need);
  if (was_reset) {  // the new episode's layout
    store_cells(S, u, x, a, b);
    pack_obs_cells(S, x);
  } else if (MODE == MODE_ATK && u.cells_dirty) {
    // TD-atk: map[6] changed in some sub-step -- the raw words, once
    const size_t cb = (size_t)b * x.NCr;
    for (int i = x.lane; i < x.NCr; i += 64) sst(&a.cells[cb + i], raw[i] & ~kTwBits);
  }
  store_board(S, u, x, a, b, was_reset || done || u.flags != S.flags0);
  store_outputs(a, b, total, ep_ret, real_def, ep_steps, fail_def, done, win, allow, cool, x.lane);
  // the observation last and once: the state after the last executed sub-step
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

// One wave per board, grid B, the XCD-contiguous board map: td_step_kernel's shape.
template <int LT, int MODE, class OT>
__device__ __forceinline__ void skip_kernel_body(const StepArgs& a) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ Smem<NC> S;
  __shared__ uint32_t raw[MODE == MODE_ATK ? NC : 4];  // TD-atk: the raw cell words (skip_board)
  const int i = (int)blockIdx.x;
  prologue_args(a);
  if (i >= a.B) return;
  const int b = a.xcd_map ? xcd_board(i, a.B) : i;
  const int L = LT ? LT : a.L;
  const Ctx x{S.cfg, L, L * L, (int)(threadIdx.x & 63), a.cfgs, a.epoch};
  const uint4 cfgv = load_cfg(a.cfg, x.lane);
  Prefetch P;
  prefetch_issue<PF_LARGE, PF_LARGE>(P, a, b, x.lane, x.NCr, MODE != MODE_ATK);
  store_cfg(S, cfgv, x.lane);
  wsync();
  skip_board<NC, LT, MODE, OT>(S, raw, x, a, b, P);
}

}  // namespace td
