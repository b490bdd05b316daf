// td_playout.h -- random playouts (td_playout, td_playout_boards[_dev]): up to `steps` board
// steps of every board served, in ONE launch, under the uniform random legal policy, and no
// observation written.  Sub-step j of a board is exactly td_sample_actions at ticket + j on the
// board's state before it, then one td_step_boards step with those actions:
//
//   load               the board once, as a step loads it
//   sub-step j         cool-downs; the sampled action(s) of the side(s) the caller controls,
//                      drawn from the LDS image and applied to it; the built-in opponent on the
//                      board's own stream; cells packed; board_step; the large kernel's MT
//                      pre-draw rule -- step_board's order (td_step_body.h)
//   episode end        the board stops after the sub-step that finished its episode; with
//                      auto-reset its new episode starts there (one layout per launch), as
//                      frame skip
//   store              what skip_board stores after its loop, minus everything that serves
//                      the observation: no dirty classes, no group statistics, no broadcast
//                      channels, no writers
//
// The draw (playout_defender, playout_attacker) is td_sample.h's rule over td_mask.h's verdicts,
// counted by the per-op structure of the legality rule instead of a 6 L^2-byte row: the build
// candidates of the four tower types are one cell set (map[6] == 0), each type gated by one
// price compare and the tower capacity; the level-up and destruct candidates are the cells that
// carry a tower, whose type and level are the tower nibble of the LDS cell word.  Three ballot
// counts per 64 cells give the six per-op counts, the pick's op follows from them, and one more
// pass of ballots finds the r-th cell of that op's set: ascending a = op L^2 + cell, as the
// sampler's row walk.  The raw cell words (map[6] in bits 24-31, the nibble in bits 10-13) are
// kept beside the packed ones, skip_board's TD-atk arrangement in all three modes here: swapped
// in for the sub-steps whose defender -- sampled or built in -- is off cool-down, and written
// back once if map[6] changed.
//
// What belongs here: playout_board and the kernels' body.  The kernels and their rows are
// td_playout.hip's; skip_board and step_board share no text with this path beyond the pieces it
// calls.  The probes (td_probe.h) run playout_board with PROBE set: the same sub-steps on a board
// that is only read.
#pragma once
#include "td_list_dev.h"
#include "td_mask.h"
#include "td_sample.h"
#include "td_step_body.h"
#include "td_step_skip.h"

namespace td {

// The sampled defender action on the board image (raw cell words in S.cell): op << 10 | cell of
// the action a = op L^2 + cell, or -1 where the defender does nothing (cool-down closed, nothing
// legal, the idle draw fired).
template <int NC>
__device__ __forceinline__ int playout_defender(const Smem<NC>& S, const U& u, const Ctx& x, uint64_t key, uint64_t ub,
                                                uint32_t idle) {
  if (u.def_cd != 0) return -1;  // (after the decrement: mask_cd_open of the header's value)
  const TdDevCfg& C = x.C;
  const int nt = u.nt < TCAP ? u.nt : TCAP;
  // a cell's three memberships: build (any type), level-up, destruct
  auto classes = [&](int c, bool& e, bool& up, bool& de) {
    const bool in = c < x.NCr;
    const uint32_t w = in ? S.cell[c] : 0u;
    const uint32_t nib = (w >> 10) & 0xFu;
    const bool has = in && (nib & 8u) != 0u;
    // the tower word's type and level bits, as load_board and the tower operations keep them
    const uint32_t ti = ((nib & 3u) << 12) | (((nib >> 2) & 1u) << 14);
    e = in && mask_build_code(0.0, 0.0, w, nt) == FC_OK;
    up = mask_lvup_code(has, ti, u.cost_def, C) == FC_OK;
    de = mask_destruct_code(has) == FC_OK;
  };
  int n_e = 0, n_up = 0, n_de = 0;
  for (int base = 0; base < x.NCr; base += 64) {
    bool e, up, de;
    classes(base + x.lane, e, up, de);
    n_e += popc64(ballot(e));
    n_up += popc64(ballot(up));
    n_de += popc64(ballot(de));
  }
  int cnt[6];
#pragma unroll
  for (int t = 0; t < 4; ++t) cnt[t] = u.cost_def < C.t_price[t][0] ? 0 : n_e;  // FC_COST first, as mask_build_code
  cnt[4] = n_up;
  cnt[5] = n_de;
  const int n_def = cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4] + cnt[5];
  if (sample_idles(sample_u(key, ub, SAMPLE_DEF_IDLE), idle, n_def)) return -1;
  int r = sample_pick(sample_u(key, ub, SAMPLE_DEF_PICK), n_def);
  int op = 0;
#pragma unroll
  for (int t = 0; t < 5; ++t)
    if (op == t && r >= cnt[t]) { r -= cnt[t]; op = t + 1; }
  // the r-th cell of op's set, in ascending order
  int cell = 0;
  for (int base = 0; base < x.NCr; base += 64) {
    bool e, up, de;
    classes(base + x.lane, e, up, de);
    uint64_t m = ballot(op < 4 ? e : (op == 4 ? up : de));
    const int c = popc64(m);
    if (r >= c) { r -= c; continue; }
    for (; r > 0; --r) m &= m - 1ull;
    cell = base + ctz64(m);
    break;
  }
  return (op << 10) | cell;
}

// The sampled attacker pair road * 4 + type, or -1: the 12 verdicts are one ballot, as the
// sampler's.
__device__ __forceinline__ int playout_attacker(const U& u, const Ctx& x, uint64_t key, uint64_t ub, uint32_t idle) {
  const TdDevCfg& C = x.C;
  bool ok = false;
  // (atk_cd after the decrement: 1 stands for every value mask_cd_open refuses)
  if (x.lane < 12)
    ok = mask_summon_ok(x.lane >> 2, x.lane & 3, mask_enemy_lv(u.steps, C), u.num_roads, u.atk_cd == 0 ? 0 : 2, u.n,
                        u.cost_atk, C);
  uint32_t m = (uint32_t)ballot(ok) & 0xfffu;
  const int n_atk = __popc(m);
  if (sample_idles(sample_u(key, ub, SAMPLE_ATK_IDLE), idle, n_atk)) return -1;
  for (int k = sample_pick(sample_u(key, ub, SAMPLE_ATK_PICK), n_atk); k > 0; --k) m &= m - 1u;
  return __builtin_ctz(m);
}

// PROBE (td_probe.h): the same sub-steps on a board that is only read.  The opponent's stream runs
// on `mt`, the wave's private copy of the board's 624 words (its lazy twists land there), the
// outputs go to row `row` of the caller's [B][reps] buffers, and nothing of the handle is written:
// no reset, no flag, no board, stream or episode store.
template <int NC, int LT, int MODE, bool PROBE = false>
__device__ __forceinline__ void playout_board(Smem<NC>& S, uint32_t* raw, const Ctx& x, const StepArgs& a,
                                              const PlayoutArgs& p, int b, const Prefetch& P, uint32_t* mt = nullptr,
                                              int row = 0) {
  const TdDevCfg& C = x.C;
  uint32_t* const opp = PROBE ? mt : a.opp_mt + (size_t)b * OPP_WORDS;
  const int o = PROBE ? row : b;  // the outputs' row
  uint32_t* const hot = a.opp_hot + (size_t)b * HOT_WORDS;
  U u;
  load_board<NC, PF_LARGE, PF_LARGE>(S, u, x, a, b, P);
  WaveMt R{opp, lane_word(P.w, PF_HOT + 0), lane_word(P.w, PF_HOT + 1)};
  R.cn = lane_word(P.w, PF_HOT + 2);
  R.cbase = lane_word(P.w, PF_HOT + 3);
  R.cache = __shfl(P.w, PF_HOT + 4 + (x.lane < HOT_CACHE ? x.lane : 0));
  const int64_t empty_def = (int64_t)6 * x.NCr;
  if (!mask_board_live(u.num_roads)) {
    // never reset (its road generation failed): nothing to play, every output defined
    if (x.lane == 0) {
      if (!PROBE) a.hdr[b].flags = u.flags | FLAG_NO_LAYOUT;
      a.reward[o] = 0.0;
      a.done[o] = 1;
      if (p.steps_run) p.steps_run[o] = 0;
      if (a.win) a.win[o] = -1;
      if (PROBE) {
        if (p.first_def) p.first_def[o] = empty_def;
      } else {
      if (a.allow_next) a.allow_next[b] = 0;
      if (a.cooldowns) a.cooldowns[b] = 0;
      if (a.ep_return) a.ep_return[b] = 0.0;
      if (a.ep_len) a.ep_len[b] = 0;
      if (p.first_def) p.first_def[b] = empty_def;  // what the sampler gives such a board
      }
    }
    if (p.first_atk && x.lane < 24) p.first_atk[(size_t)o * 24 + x.lane] = 4;
    return;
  }

  const uint64_t ub = (uint64_t)(uint32_t)b;
  double total = 0.0;
  bool done = false, refilled = false;
  const int k = a.frame_skip;
  int j = 0;
#pragma unroll 1
  for (; j < k; ++j) {
    u.atk_cd = u.atk_cd - 1 > 0 ? u.atk_cd - 1 : 0;
    u.def_cd = u.def_cd - 1 > 0 ? u.def_cd - 1 : 0;
    // the sub-step's key: one wave-uniform splitmix over the host's sm(seed)
    const uint64_t key = sample_sm(p.key0 + p.ticket + (uint64_t)(uint32_t)j);
    // the cell words are raw in sub-step 0 (as loaded); later only while a defender may act
    const bool raw_cells = j == 0 || u.def_cd == 0;
    if (j > 0 && raw_cells) skip_copy_cells<NC>(S.cell, raw, x.NCr, x.lane);
    // ---- the sampled actions, both from the state before the sub-step (the defender's
    // operation changes nothing the attacker's verdicts read, so the order is free)
    int act_def = -1, act_atk = -1;
    if (MODE != MODE_ATK) act_def = playout_defender(S, u, x, key, ub, p.def_idle);
    if (MODE != MODE_DEF) act_atk = playout_attacker(u, x, key, ub, p.atk_idle);
    if (j == 0) {
      if (MODE != MODE_ATK && p.first_def && x.lane == 0) p.first_def[o] = act_def >= 0 ? (int64_t)((act_def >> 10) * x.NCr + (act_def & 1023)) : empty_def;
      if (MODE != MODE_DEF && p.first_atk && x.lane < 24)
        p.first_atk[(size_t)o * 24 + x.lane] =
            act_atk >= 0 && x.lane == (act_atk >> 2) * 8 ? (int64_t)(act_atk & 3) : (int64_t)4;
    }
    // ---- defender (step_board: legal by construction, FailCode 0)
    if (MODE != MODE_ATK && act_def >= 0) {
      if (defender_op(S, u, x, act_def >> 10, act_def & 1023) == FC_OK) u.def_cd = C.def_interval;
    }
    // ---- attacker: the one-enemy cluster (t, 4 x 7) on the chosen road (attacker_actions)
    if (MODE != MODE_DEF && act_atk >= 0) {
      summon_cluster(S, u, x, (uint32_t)(act_atk & 3) | 0x44444440u, act_atk >> 2, nullptr);
      u.atk_cd = C.atk_interval;
      wsync();
    }
    // ---- the built-in opponent
    // (a probe: the board's own stream only -- random_agent = 0 is refused, and its branch would
    // store to the layout stream)
    if constexpr (PROBE) {
      OppRng<false> G{R, R};
      if (MODE == MODE_DEF) opponent_enemy(S, u, x, G, a.difficulty);
      if (MODE == MODE_ATK && raw_cells) opponent_tower(S, u, x, G, a.difficulty);
    } else {
      if (MODE == MODE_DEF) with_opp_rng(a, b, x.lane, R, [&](auto& G) { opponent_enemy(S, u, x, G, a.difficulty); });
      if (MODE == MODE_ATK && raw_cells)
        with_opp_rng(a, b, x.lane, R, [&](auto& G) { opponent_tower(S, u, x, G, a.difficulty); });
    }
    // the towers and map[6] are final for this sub-step: the raw words aside, then packed
    if (raw_cells) {
      skip_copy_cells<NC>(raw, S.cell, x.NCr, x.lane);
      pack_obs_cells(S, x);
    }
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
    if (done) { ++j; break; }
  }

  // ---- what the last executed sub-step would have written
  const int ep_steps = u.steps;
  int8_t win = -1;
  if (done) {
    if (MODE == MODE_ATK) win = u.base_LP <= 0 ? 1 : 0;
    else win = u.base_LP > 0 ? 1 : 0;
  }
  if constexpr (PROBE) {
    // the outputs only: the board, its stream, its episode records and its layouts stay as they are
    if (x.lane == 0) {
      sst(&a.reward[o], total);
      sst(&a.done[o], (uint8_t)(done ? 1 : 0));
      if (a.win) sst(&a.win[o], win);
      if (p.steps_run) sst(&p.steps_run[o], (int32_t)j);
    }
    return;
  }
  const uint8_t allow = (uint8_t)((u.atk_cd <= 1 ? 1 : 0) | (u.def_cd <= 1 ? 2 : 0));
  const int acd = u.atk_cd < 15 ? u.atk_cd : 15, dcd = u.def_cd < 15 ? u.def_cd : 15;
  const uint8_t cool = (uint8_t)(acd | (dcd << 4));
  const double ep_ret = u.ep_ret;

  if (done) u.episodes += 1;
  bool was_reset = false;
  uint32_t lay_head = 0;
  if (done && a.autoreset && !a.opp_np) {
    // at most one staged layout per launch (skip_board)
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
    if (p.steps_run) sst(&p.steps_run[b], (int32_t)j);
  }
  if (refilled && x.lane < HOT_CACHE) sst(&hot[4 + x.lane], R.cache);
  if (was_reset) {  // the new episode's layout
    store_cells(S, u, x, a, b);
  } else if (u.cells_dirty) {
    // map[6] changed in some sub-step -- the raw words, once
    const size_t cb = (size_t)b * x.NCr;
    for (int i = x.lane; i < x.NCr; i += 64) sst(&a.cells[cb + i], raw[i] & ~kTwBits);
  }
  store_board(S, u, x, a, b, was_reset || done || u.flags != S.flags0);
  store_outputs(a, b, total, ep_ret, empty_def, ep_steps, 0, done, win, allow, cool, x.lane);
}

// One wave per entry, one board per workgroup, the XCD-contiguous entry map: step_sel_body's
// shape.  The entries are p.ids[0 .. n) with n as td_list_dev.h makes it, or every board
// (p.ids == nullptr: entry i is board i, n = a.B).
template <int LT, int MODE>
__device__ __forceinline__ void playout_kernel_body(const StepArgs& a, const PlayoutArgs& p) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ Smem<NC> S;
  __shared__ uint32_t raw[NC];  // the raw cell words (playout_board)
  const int i = (int)blockIdx.x;
  prologue_args(a);
  const int n = p.ids ? list_length(p.cap, p.count, p.verdict) : a.B;
  if (i >= n) return;
  const int e = a.xcd_map ? xcd_board(i, n) : i;
  const int b = p.ids ? list_word(p.ids, e) : e;
  const int L = LT ? LT : a.L;
  const Ctx x{S.cfg, L, L * L, (int)(threadIdx.x & 63), a.cfgs, a.epoch};
  const uint4 cfgv = load_cfg(a.cfg, x.lane);
  Prefetch P;
  prefetch_issue<PF_LARGE, PF_LARGE>(P, a, b, x.lane, x.NCr, false);
  store_cfg(S, cfgv, x.lane);
  wsync();
  playout_board<NC, LT, MODE>(S, raw, x, a, p, b, P);
}

}  // namespace td
