// td_step_rules.h -- the game rules of one env step, on a board staged in LDS.
// What belongs here: the defender's tower operations and the multi-action scan
// (TDBoard.py:226-293), the attacker's clusters (summon_cluster, attacker_actions) and
// TDBoard.step itself (board_step).  Each takes the board (Smem, U, Ctx of
// td_step_state.h) and changes it; none touches HBM except to read the actions.
#pragma once
#include "td_board.h"
#include "td_kernels.h"
#include "td_step_state.h"
#include "td_wave.h"

namespace td {

// ---------------------------------------------------------------------------
// defender operations (TDBoard.py:226-293), wave-uniform
// ---------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void diamond(Smem<NC>& S, const Ctx& x, int cell, int delta) {
  const int k = x.C.tower_distance, W = 2 * k + 1, L = x.L;
  const int r0 = div_side(cell, x.Lm), c0 = cell - r0 * L;
  for (int idx = x.lane; idx < W * W; idx += 64) {
    int i = idx / W - k, j = idx % W - k;
    int ai = i < 0 ? -i : i, aj = j < 0 ? -j : j;
    int r = r0 + i, c = c0 + j;
    if (ai + aj <= k && r >= 0 && r < L && c >= 0 && c < L) {
      uint32_t w = S.cell[r * L + c];
      int cnt = (int)(w >> 24) + delta;
      S.cell[r * L + c] = (w & 0x00ffffffu) | ((uint32_t)(cnt & 0xff) << 24);
    }
  }
  wsync();
}

template <int NC>
__device__ __forceinline__ int tower_build(Smem<NC>& S, U& u, const Ctx& x, int t, int cell) {
  const double price = x.C.t_price[t][0];
  if (u.cost_def < price) return FC_COST;                 // :228
  if (cw_block(S.cell[cell]) > 0) return FC_POS;          // :232
  if (u.nt >= TCAP) { u.flags |= FLAG_TW_OVERFLOW; return FC_CAP; }
  if (x.lane == 0) {
    S.tInf[u.nt] = tw_pack(cell, t, 0, x.ep, x.ep);
    S.tCd[u.nt] = 0.0;
    set_tower(S, cell, tw_nib(0, t));
  }
  u.nt += 1;
  u.cost_def = dsub(u.cost_def, price);                   // :238
  u.cells_dirty = true;
  u.tw_dirty = true;
  wsync();
  diamond(S, x, cell, +1);                                // :239-245
  return FC_OK;
}

template <int NC>
__device__ __forceinline__ int find_tower(Smem<NC>& S, const U& u, const Ctx& x, int cell) {
  bool hit = x.lane < u.nt && (int)(S.tInf[x.lane] & 0xfffu) == cell;
  uint64_t m = ballot(hit);
  return m ? ctz64(m) : -1;
}

template <int NC>
__device__ __forceinline__ int tower_lvup(Smem<NC>& S, U& u, const Ctx& x, int cell) {
  int k = find_tower(S, u, x, cell);
  if (k < 0) return FC_TARGET;                            // :269-271
  uint32_t ti = S.tInf[k];
  int t = (ti >> 12) & 3, lv = (ti >> 14) & 1;
  if (lv >= x.C.max_tower_lv) return FC_LVMAX;            // :252
  double price = x.C.t_price[t][lv + 1];                  // :256
  if (u.cost_def < price) return FC_COST;
  wsync();
  if (x.lane == 0) {
    S.tInf[k] = tw_pack(cell, t, lv + 1, tw_ec(ti), x.ep);
    set_tower(S, cell, tw_nib(lv + 1, t));
  }
  u.cost_def = dsub(u.cost_def, price);                   // :266
  u.tw_dirty = true;
  wsync();
  return FC_OK;
}

template <int NC>
__device__ __forceinline__ int tower_destruct(Smem<NC>& S, U& u, const Ctx& x, int cell) {
  int k = find_tower(S, u, x, cell);
  if (k < 0) return FC_TARGET;                            // :291-293
  uint32_t ti = S.tInf[k];
  int t = (ti >> 12) & 3, lv = (ti >> 14) & 1;
  // Tower.cost: tower_cost[t][0] when built, + tower_attack_interval[t][1] at the upgrade
  // (the upgrade_tower argument swap), each from the epoch it was captured in
  double value = captured(x, tw_ec(ti), [&](const TdDevCfg& c) { return c.t_price[t][0]; });
  if (lv >= 1) value = dadd(value, captured(x, tw_eu(ti), [&](const TdDevCfg& c) { return c.t_addcost[t][lv]; }));
  u.cost_def = dadd(u.cost_def, dmul(value, x.C.destruct_return));  // :276
  u.cost_def = pymin(u.cost_def, u.max_cost);                      // :277
  u.cells_dirty = true;
  u.tw_dirty = true;
  // towers.remove(t): keep the order of the rest (:278)
  uint32_t vi = 0;
  double vc = 0.0;
  int j = x.lane;
  if (j >= k && j + 1 < u.nt) { vi = S.tInf[j + 1]; vc = S.tCd[j + 1]; }
  wsync();
  if (j >= k && j + 1 < u.nt) { S.tInf[j] = vi; S.tCd[j] = vc; }
  if (x.lane == 0) set_tower(S, cell, 0u);
  u.nt -= 1;
  wsync();
  diamond(S, x, cell, -1);                                // :281-287
  return FC_OK;
}

template <int NC>
__device__ __forceinline__ int defender_op(Smem<NC>& S, U& u, const Ctx& x, int op, int cell) {
  if (op < 4) return tower_build(S, u, x, op, cell);
  if (op == 4) return tower_lvup(S, u, x, cell);
  return tower_destruct(S, u, x, cell);
}

// Multi-action defender: the serial (r, c, t) scan of TDDefense.py:42-60 /
// TDMulti.py:209-227.  The (6, L, L) int64 flags are read first with 16-B loads
// (8 in flight per lane) and folded into one 6-bit flag byte per cell in LDS (the
// group map grp[0], unused until enemy_stats).  Cells where no operation can change
// the board are skipped: per 64-cell chunk a ballot marks the cells whose flagged
// build / lvup / destruct would succeed in the CURRENT state, the first such cell
// runs the reference's exact serial sequence, and the ballot is recomputed.
// Skipped cells would only have produced failures, which leave no trace in
// multi-action mode.  The real actions (grp[1]) go out as int64 (6, L, L) in
// 128-B-aligned windows, like the observation.
// (In the two-wave kernel the second wave folds the flags while the first loads the
// board, and writes the real actions out after the step's actions: scan_fold /
// scan_write_real below, handed over at barriers.)
// The flags folded into grp[0] (grp[1] cleared); true when a flag is not 0 / 1 / 2.
template <int NC>
__device__ __forceinline__ bool scan_fold(Smem<NC>& S, int lane, int ncr, const int64_t* A) {
  const int n = 6 * ncr;
  uint8_t* flag = &S.grp[0][0];
  uint32_t* fw = reinterpret_cast<uint32_t*>(flag);
  for (int i = lane; i < (2 * NC) / 4; i += 64) fw[i] = 0u;  // grp[0] and grp[1]
  wsync();
  bool bad = false;
  if ((ncr & 1) == 0 && (reinterpret_cast<uintptr_t>(A) & 15u) == 0) {  // 16-B units of two cells of one plane
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    const i64x2* A2 = reinterpret_cast<const i64x2*>(A);
    const int n2 = n / 2;
    constexpr int K = 8;  // 16-B loads in flight per lane
    // (not unrolled: with the trip count known (NC) the compiler unrolled this loop and
    // hoisted the next rounds' loads, 85-91 VGPRs at 20x20 and 182-188 at 30x30 in every
    // multi-action kernel; rolled, 62-63)
#pragma unroll 1
    for (int base = 0; base < n2; base += 64 * K) {
      i64x2 v[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = base + 64 * k + lane;
        v[k] = e < n2 ? __builtin_nontemporal_load(A2 + e) : i64x2{0, 0};
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int e = base + 64 * k + lane;
        if (e < n2) {
          const int pl = (2 * e) / ncr, c = 2 * e - pl * ncr;
          bad |= (unsigned long long)v[k].x > 2ull || (unsigned long long)v[k].y > 2ull;
          const uint32_t bits = ((v[k].x == 1 ? 1u : 0u) << (8 * (c & 3)) | (v[k].y == 1 ? 1u : 0u) << (8 * ((c + 1) & 3)))
                                << pl;
          if (bits) atomicOr(&fw[c >> 2], bits);
        }
      }
    }
  } else {
    for (int e = lane; e < n; e += 64) {
      const int64_t v = A[e];
      const int pl = e / ncr, c = e - pl * ncr;
      bad |= v < 0 || v > 2;
      if (v == 1) atomicOr(&fw[c >> 2], (1u << pl) << (8 * (c & 3)));
    }
  }
  const bool any_bad = ballot(bad) != 0ull;
  wsync();
  return any_bad;
}

// The real actions (grp[1]) out as int64 (6, L, L) in 128-B-aligned windows.
template <int NC>
__device__ __forceinline__ void scan_write_real(const Smem<NC>& S, int lane, int ncr, int64_t* R) {
  const int n = 6 * ncr;
  const uint8_t* real = &S.grp[1][0];
  if ((ncr & 1) == 0 && (reinterpret_cast<uintptr_t>(R) & 15u) == 0) {
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    i64x2* R2 = reinterpret_cast<i64x2*>(R);
    const int n2 = n / 2, mis = (int)((reinterpret_cast<uintptr_t>(R2) >> 4) & 7u);
    for (int e = lane - mis; e < n2; e += 64) {
      if (e < 0) continue;
      const int pl = (2 * e) / ncr, c = 2 * e - pl * ncr;
      const uint32_t r2 = *reinterpret_cast<const uint16_t*>(real + c);
      __builtin_nontemporal_store(i64x2{(long long)((r2 >> pl) & 1u), (long long)((r2 >> (8 + pl)) & 1u)}, R2 + e);
    }
  } else {
    for (int e = lane; e < n; e += 64) {
      const int pl = e / ncr;
      R[e] = (real[e - pl * ncr] >> pl) & 1u;
    }
  }
}

// FOLD: the flags are folded here (else by the second wave, `bad` its verdict); WRITE:
// the real actions are written here (else by the second wave after barrier (A)).
template <int NC, bool FOLD = true, bool WRITE = true>
__device__ __forceinline__ void defender_scan(Smem<NC>& S, U& u, const Ctx& x, const int64_t* A, int64_t* R, bool active,
                                              bool bad = false) {
  const TdDevCfg& C = x.C;
  const int ncr = x.NCr;
  uint8_t* flag = &S.grp[0][0];
  uint8_t* real = &S.grp[1][0];
  if constexpr (FOLD) bad = scan_fold(S, x.lane, ncr, A);
  if (bad) u.flags |= FLAG_BAD_ACTION;
  for (int base = 0; base < ncr && active; base += 64) {
    const int cell = base + x.lane;
    const bool valid = cell < ncr;
    const uint32_t fl = valid ? flag[cell] : 0u;
    int last = -1;
    while (true) {
      bool cand = false;
      if (valid && fl && x.lane > last) {
        uint32_t w = S.cell[cell];
        uint32_t tw = twr_of(w);
        bool canb = false;
        if (cw_block(w) == 0) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (((fl >> t) & 1u) && !(u.cost_def < C.t_price[t][0])) canb = true;
        }
        bool hasT = (tw & 0x80u) != 0;
        int tlv = (tw >> 2) & 1, tty = tw & 3;
        bool canl = hasT && ((fl >> 4) & 1u) && tlv < C.max_tower_lv && !(u.cost_def < C.t_price[tty][tlv + 1]);
        bool cand_d = hasT && ((fl >> 5) & 1u);
        cand = canb || canl || cand_d;
      }
      uint64_t m = ballot(cand);
      if (!m) break;
      const int j = ctz64(m);
      const int c = base + j;
      const uint32_t f = rdl(fl, j);
      uint32_t rb = 0;
      for (int t = 0; t < 4; ++t)
        if ((f >> t) & 1u)
          if (tower_build(S, u, x, t, c) == FC_OK) { rb |= 1u << t; u.def_cd = C.def_interval; }
      if ((f >> 4) & 1u)
        if (tower_lvup(S, u, x, c) == FC_OK) { rb |= 16u; u.def_cd = C.def_interval; }
      if ((f >> 5) & 1u)
        if (tower_destruct(S, u, x, c) == FC_OK) { rb |= 32u; u.def_cd = C.def_interval; }
      if (x.lane == j) real[c] = (uint8_t)rb;
      last = j;
    }
  }
  wsync();
  if (WRITE && R) scan_write_real(S, x.lane, ncr, R);
}

// ---------------------------------------------------------------------------
// attacker: summon_cluster (TDBoard.py:199-224)
// ---------------------------------------------------------------------------
// Cluster types / real actions are packed 4 bits per slot (slot k at bits 4k..4k+3).
template <int NC>
__device__ __forceinline__ int summon_cluster(Smem<NC>& S, U& u, const Ctx& x, uint32_t types, int road, uint32_t* real) {
  const TdDevCfg& C = x.C;
  // progress >= enemy_upgrade_at (:201) as an integer test: u.progress is steps / max_episode_steps
  // wherever a cluster is summoned (after load_board, reset_board and each board_step), and that
  // quotient passes the threshold from upgrade_step on (td_upgrade_step.h)
  // (a threshold no step count reaches gives INT32_MAX: the two tests then differ at steps ==
  // INT32_MAX alone, the last value the int32 counter can hold)
  const int lv = u.steps >= C.upgrade_step ? 1 : 0;
  const int st = u.start(road);
  if (x.short_cuts && (types & 0xfu) <= 4u && types == (types & 0xfu) * 0x11111111u) {
    // Eight equal types (the lv1 opponent always; an empty or a one-type cluster of a caller):
    // the first slot that fails -- the cost, or a full list with its flag -- leaves cost_atk and
    // the list as they were, so every later slot fails the same way.  Cost and max LP are read
    // once, and the summoned enemies are written one per lane.
    const int t = (int)(types & 0xfu);
    if (t == 4) {  // nothing tried (:207-209)
      if (real) *real = types;
      return FC_OK;
    }
    const double cost = C.e_cost[t][lv], lp = C.e_lp[t][lv];
    const int n0 = u.n;
    int m = 0;
    while (m < 8 && !(u.cost_atk < cost)) {                 // :212-213
      if (n0 + m >= ECAP) { u.flags |= FLAG_EN_OVERFLOW; break; }
      u.cost_atk = dsub(u.cost_atk, cost);                  // :215
      m += 1;
    }
    if (x.lane < m) {
      S.eLP[n0 + x.lane] = lp;
      S.eMg[n0 + x.lane] = 0.0;
      S.eInf[n0 + x.lane] = en_pack(st, t, lv, 0, x.ep);
    }
    if (m) {
      u.n = n0 + m;
      u.en_touch = true;  // a new enemy: its group's planes change
    }
    if (real) {
      const uint32_t keep = m >= 8 ? ~0u : (1u << (4 * m)) - 1u;
      *real = (types & keep) | (0x44444444u & ~keep);
    }
    return m ? FC_OK : FC_COST;                             // :219-224
  }
  bool tried = false, summoned = false;
  uint32_t rp = 0;
  // the four types' cost (lanes 0-3) and max LP (lanes 4-7) at this level in ONE LDS read,
  // then read per slot from those lanes (8 dependent LDS round trips before, one per slot)
  const double tab = x.lane < 4 ? C.e_cost[x.lane & 3][lv] : C.e_lp[x.lane & 3][lv];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int t = (int)((types >> (4 * k)) & 0xfu);
    int r = t;
    if (t != 4) {                                           // :207-209
      tried = true;
      const double cost = rdl(tab, t);
      if (u.cost_atk < cost) {                              // :212-213
        r = 4;
      } else if (u.n >= ECAP) {
        u.flags |= FLAG_EN_OVERFLOW;
        r = 4;
      } else {
        u.cost_atk = dsub(u.cost_atk, cost);                // :215
        const double lp = rdl(tab, 4 + t);
        if (x.lane == 0) {
          S.eLP[u.n] = lp;
          S.eMg[u.n] = 0.0;
          S.eInf[u.n] = en_pack(st, t, lv, 0, x.ep);
        }
        u.n += 1;
        u.en_touch = true;  // a new enemy: its group's planes change
        summoned = true;
      }
    }
    rp |= (uint32_t)r << (4 * k);
  }
  if (real) *real = rp;
  return (tried && !summoned) ? FC_COST : FC_OK;            // :219-224
}

// ---------------------------------------------------------------------------
// TDBoard.step (TDBoard.py:295-368) + enemy_LP statistics
// ---------------------------------------------------------------------------
// Enemy.defense as the enemy captured it (TDElements.py:33-43)
__device__ __forceinline__ double e_def(const Ctx& x, uint32_t inf) {
  const int t = en_type(inf), lv = en_lv(inf);
  return captured(x, en_ep(inf), [&](const TdDevCfg& c) { return c.e_def[t][lv]; });
}

// Enemies up to which the towers target in parallel (board_step; FEW = false: never --
// the large kernel, where it measured slower, and the two-wave 20x20 single-action
// kernel, which has no registers to spare for it).
constexpr int kFewEnemies = 16;

template <int NC, bool FEW = true>
__device__ __forceinline__ double board_step(Smem<NC>& S, U& u, const Ctx& x, const StepArgs& a, int b) {
  const TdDevCfg& C = x.C;
  const int L = x.L, lane = x.lane;
  double reward = dadd(0.0, C.reward_time);                 // :298-299
  u.steps += 1;                                             // :300
  u.progress = ddiv((double)u.steps, (double)C.max_episode_steps);  // :301

  // --- stable sort by f64 key dist - margin (:305): rank = #smaller + #equal-before
  const int n = u.n;
  double lp[2], mg[2];
  uint32_t inf[2];
  bool val[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    int i = lane + 64 * s;
    val[s] = i < n;
    lp[s] = val[s] ? S.eLP[i] : 0.0;
    mg[s] = val[s] ? S.eMg[i] : 0.0;
    inf[s] = val[s] ? S.eInf[i] : 0u;
  }
  if (n > 1) {  // (a list of 0 or 1 enemies is sorted; most boards, most steps)
    double key[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) key[s] = val[s] ? dsub((double)pk_dist(S.cell[en_cell(inf[s])]), mg[s]) : 0.0;
    int rank[2] = {0, 0};
    for (int j = 0; j < n; ++j) {  // enemy j's key from the lane that holds it
      const double kj = j < 64 ? rdl(key[0], j) : rdl(key[1], j - 64);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        int i = lane + 64 * s;
        if (kj < key[s] || (kj == key[s] && j < i)) rank[s] += 1;
      }
    }
    // The sort is the identity on almost every board (enemies enter in order and keep it): the
    // lanes hold the sorted list already, no scatter through LDS.  A sort that moves an enemy
    // changes the order a group's LP ratios are summed in (enemy_stats).
    if (ballot((val[0] && rank[0] != lane) || (val[1] && rank[1] != lane + 64)) != 0ull) {
      u.en_touch = true;
      wsync();
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (val[s]) { S.eLP[rank[s]] = lp[s]; S.eMg[rank[s]] = mg[s]; S.eInf[rank[s]] = inf[s]; }
      wsync();
      // lane owns sorted enemies lane and lane + 64
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        int i = lane + 64 * s;
        lp[s] = val[s] ? S.eLP[i] : 0.0;
        mg[s] = val[s] ? S.eMg[i] : 0.0;
        inf[s] = val[s] ? S.eInf[i] : 0u;
      }
    }
  }

  // --- towers fire in list order (:306-313); dead enemies stay targetable.
  // Tower k lives in lane k (cool-down in a register); a fired tower is read
  // with a wave-uniform lane index (v_readlane).
  double tcd = lane < u.nt ? S.tCd[lane] : 0.0;
  const uint32_t tinf_l = lane < u.nt ? S.tInf[lane] : 0u;
  if (n == 0) {
    // no enemy anywhere: every tower just cools down (cd -= 1; no target; clamp at 0)
    if (lane < u.nt) { const double cd = dsub(tcd, 1.0); tcd = cd > 0.0 ? cd : 0.0; }
  } else {
    // Targeting never depends on another tower's shot (dead enemies stay targetable), so
    // what the serial loop needs per tower -- range, interval, attack and splash as the
    // tower captured them -- is gathered once, one tower per lane, into the enemy
    // arrays' LDS (dead between the sorted load above and the compaction below): the
    // loop reads it with one uniform-address LDS load per value, no epoch branches.
    double* const tp = S.eLP;  // [TCAP][4]: rge, intv, atk, dmgrge
    static_assert(sizeof(S.eLP) >= TCAP * 4 * sizeof(double), "tower table in the enemy LP array");
    if (lane < u.nt) {
      const int tt = (tinf_l >> 12) & 3, tl = (tinf_l >> 14) & 1, te = tw_eu(tinf_l);
      tp[4 * lane + 0] = captured(x, te, [&](const TdDevCfg& c) { return c.t_rge[tt][tl]; });
      tp[4 * lane + 1] = captured(x, te, [&](const TdDevCfg& c) { return c.t_intv[tt][tl]; });
      tp[4 * lane + 2] = captured(x, te, [&](const TdDevCfg& c) { return c.t_atk[tt][tl]; });
      tp[4 * lane + 3] = captured(x, te, [&](const TdDevCfg& c) { return c.t_dmg[tt][tl]; });
    }
    wsync();
    if (FEW && n <= kFewEnemies) {
      // A few enemies (most boards that have any): the towers pick their targets in
      // parallel, lane k = tower k, each scanning the n enemies in list order; then the
      // shots land in tower order, each enemy (lane j) taking the hits of the towers that
      // fired, one tower after the other -- the reference's order of LP updates per enemy
      // (:306-313), without a dependent LDS round trip per tower.
      const bool tk = lane < u.nt;
      const int tt = (int)((tinf_l >> 12) & 3u), tc = (int)(tinf_l & 0xfffu);
      double cd = dsub(tcd, 1.0);                            // :307
      const bool tries = tk && !(cd > 0.0);
      const double rge = tries ? tp[4 * lane] : -1.0;
      int tgt = -1;
      for (int j = 0; j < n; ++j) {  // first enemy within range (list order)
        const int ec = en_cell(rdl(inf[0], j));
        if (tgt < 0 && (double)cheb(ec, tc, L, x.Lm) <= rge) tgt = j;
      }
      const int tgc = en_cell((uint32_t)__shfl((int)inf[0], tgt < 0 ? 0 : tgt));  // every lane shuffles
      const double dr = tt >= 2 && tgt >= 0 ? tp[4 * lane + 3] : -1.0;
      int frz = -1;  // TowerFrozen: the first enemy within splash of the target (:112-132)
      if (tt == 3)
        for (int j = 0; j < n; ++j) {
          const int ec = en_cell(rdl(inf[0], j));
          if (frz < 0 && (double)cheb(tgc, ec, L, x.Lm) <= dr) frz = j;
        }
      if (tgt >= 0) cd = dadd(cd, tp[4 * lane + 1]);         // cd += intv
      if (tries && cd < 0.0) cd = 0.0;                       // :311-312
      if (tk) tcd = cd;
      const uint32_t slow = (uint32_t)C.frozen_time << 16;   // config.frozen_time, read live (:126)
      uint64_t fm = ballot(tgt >= 0);
      if (fm) u.en_touch = true;  // a shot lands: LP, a kill or a slow-down with its LP loss
      for (; fm; fm &= fm - 1) {  // the towers that fired, in order
        const int k = ctz64(fm);
        const int kt = (int)((rdl(tinf_l, k) >> 12) & 3u);
        const double atk = tp[4 * k + 2];
        if (kt <= 1) {  // TowerArrow / TowerMagic (TDElements.py:71-93)
          if (lane == (int)rdl((uint32_t)tgt, k)) lp[0] = damage(lp[0], atk, e_def(x, inf[0]), kt == 1);
        } else if (kt == 2) {  // TowerBomb splash (:95-110)
          const int kc = (int)rdl((uint32_t)tgc, k);
          if (val[0] && (double)cheb(kc, en_cell(inf[0]), L, x.Lm) <= tp[4 * k + 3])
            lp[0] = damage(lp[0], atk, e_def(x, inf[0]), false);
        } else if (lane == (int)rdl((uint32_t)frz, k)) {
          lp[0] = damage(lp[0], atk, 0.0, true);
          inf[0] = (inf[0] & 0xff00ffffu) | slow;
        }
      }
    } else
    for (int k = 0; k < u.nt; ++k) {
      double cd = dsub(rdl(tcd, k), 1.0);                    // :307
      if (!(cd > 0.0)) {
        const uint32_t ti = rdl(tinf_l, k);
        const int tt = (ti >> 12) & 3, tc = ti & 0xfff;
        const double rge = tp[4 * k];
        bool in0 = val[0] && (double)cheb(en_cell(inf[0]), tc, L, x.Lm) <= rge;
        bool in1 = val[1] && (double)cheb(en_cell(inf[1]), tc, L, x.Lm) <= rge;
        uint64_t m0 = ballot(in0), m1 = ballot(in1);
        if (m0 | m1) {
          const int tgt = m0 ? ctz64(m0) : 64 + ctz64(m1);
          u.en_touch = true;  // a shot lands
          cd = dadd(cd, tp[4 * k + 1]);  // cd += intv
          const double atk = tp[4 * k + 2];
          if (tt <= 1) {  // TowerArrow / TowerMagic (TDElements.py:71-93)
            if (lane == (tgt & 63)) {
              if (tgt < 64) lp[0] = damage(lp[0], atk, e_def(x, inf[0]), tt == 1);
              else lp[1] = damage(lp[1], atk, e_def(x, inf[1]), tt == 1);
            }
          } else {
            const uint32_t tinf = (tgt >> 6) ? rdl(inf[1], tgt & 63) : rdl(inf[0], tgt & 63);
            const int tgc = en_cell(tinf);
            const double dr = tp[4 * k + 3];
            if (tt == 2) {  // TowerBomb splash (:95-110)
#pragma unroll
              for (int s = 0; s < 2; ++s)
                if (val[s] && (double)cheb(tgc, en_cell(inf[s]), L, x.Lm) <= dr)
                  lp[s] = damage(lp[s], atk, e_def(x, inf[s]), false);
            } else {  // TowerFrozen: first enemy within splash of the target (:112-132)
              bool h0 = val[0] && (double)cheb(tgc, en_cell(inf[0]), L, x.Lm) <= dr;
              bool h1 = val[1] && (double)cheb(tgc, en_cell(inf[1]), L, x.Lm) <= dr;
              uint64_t q0 = ballot(h0), q1 = ballot(h1);
              if (q0 | q1) {
                const int f = q0 ? ctz64(q0) : 64 + ctz64(q1);
                if (lane == (f & 63)) {
                  const uint32_t slow = (uint32_t)C.frozen_time << 16;  // config.frozen_time, read live (:126)
                  if (f < 64) { lp[0] = damage(lp[0], atk, 0.0, true); inf[0] = (inf[0] & 0xff00ffffu) | slow; }
                  else { lp[1] = damage(lp[1], atk, 0.0, true); inf[1] = (inf[1] & 0xff00ffffu) | slow; }
                }
              }
            }
          }
        }
        if (cd < 0.0) cd = 0.0;                              // :311-312
      }
      if (lane == k) tcd = cd;
    }
  }
  if (lane < u.nt) S.tCd[lane] = tcd;

  // A board without an enemy (most boards, most steps) has nobody to kill, march, leak or
  // compact: the list stays empty.  Its reward is the one the full path gives: dadd(0.0,
  // reward_time) is never -0.0, and the kill term adds reward_kill x 0 = +-0 to it (finite
  // values only: td_cfg_check.h), which changes no bit.
  if (!x.short_cuts || n != 0) {
    // --- kills (:313-317): every enemy at LP 0 was hit this step
    bool dead0 = val[0] && lp[0] == 0.0, dead1 = val[1] && lp[1] == 0.0;
    const int nk = popc64(ballot(dead0)) + popc64(ballot(dead1));
    reward = dadd(reward, dmul(C.reward_kill, (double)nk));  // :315

    // --- march (:319-344)
    bool alive[2] = {val[0] && !dead0, val[1] && !dead1};
    bool leak[2] = {false, false};
    bool walked = false;  // the enemy entered a new cell (or leaked)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (!alive[s]) continue;
      const uint32_t e = inf[s];
      const int t = en_type(e), lv = en_lv(e);
      int slow = en_slow(e), cell = en_cell(e);
      const double sp = captured(x, en_ep(e), [&](const TdDevCfg& c) { return c.e_speed[t][lv]; });
      if (slow > 0) { mg[s] = dadd(mg[s], dmul(sp, C.frozen_ratio)); slow -= 1; }
      else mg[s] = dadd(mg[s], sp);
      while (mg[s] >= 1.0) {
        walked = true;
        mg[s] = dsub(mg[s], 1.0);
        const int d = pk_dir(S.cell[cell]);
        // map[5] codes (TDBoard.py:319): 0:+c 1:-c 2:+r 3:-r
        const int r1 = div_side(cell, x.Lm);
        int r = r1 + (d == 2) - (d == 3), c = cell - r1 * L + (d == 0) - (d == 1);
        if (r < 0 || r >= L || c < 0 || c >= L) { u.flags |= FLAG_BAD_MOVE; break; }
        cell = r * L + c;
        if (cell == u.end_cell) { leak[s] = true; break; }
      }
      inf[s] = en_pack(cell, t, lv, slow, en_ep(e));
    }
    // a bad move is rare and lane-local: fold the flag into the uniform copy
    if (ballot((u.flags & FLAG_BAD_MOVE) != 0)) u.flags |= FLAG_BAD_MOVE;
    if (ballot(walked)) u.en_touch = true;
    const int nl = popc64(ballot(leak[0])) + popc64(ballot(leak[1]));
    for (int p = 0; p < nl; ++p) {                            // :336-343, in list order
      if (u.base_LP > 0) reward = dsub(reward, C.penalty_leak);
      u.base_LP = u.base_LP - 1 > 0 ? u.base_LP - 1 : 0;
    }
    // --- compact survivors, list order kept (:316-317, :345-346)
    bool keep0 = alive[0] && !leak[0], keep1 = alive[1] && !leak[1];
    const uint64_t k0 = ballot(keep0), k1 = ballot(keep1);
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    const int n2 = popc64(k0) + popc64(k1);
    wsync();
    if (keep0) { int d = popc64(k0 & lt); S.eLP[d] = lp[0]; S.eMg[d] = mg[0]; S.eInf[d] = inf[0]; }
    if (keep1) { int d = popc64(k0) + popc64(k1 & lt); S.eLP[d] = lp[1]; S.eMg[d] = mg[1]; S.eInf[d] = inf[1]; }
    u.n = n2;
  } else {
    wsync();
  }

  // --- costs (:348-353)
  double rate;
  if (u.progress >= 0.5) rate = C.atk_final_rate;
  else rate = dadd(dmul(C.atk_init_rate, dsub(1.0, u.progress)), dmul(C.atk_final_rate, u.progress));
  u.cost_atk = pymin(dadd(u.cost_atk, rate), u.max_cost);  // self.max_cost (:352-353)
  u.cost_def = pymin(dadd(u.cost_def, C.def_rate), u.max_cost);
  wsync();
  return reward;  // the caller writes the enemy list back (store_enemies)
}

// Attacker clusters of TD-atk (TDAttack.py:36-46) and TD-2p (TDMulti.py:199-206, 229-241).
template <int NC, int MODE>
__device__ __forceinline__ void attacker_actions(Smem<NC>& S, U& u, const Ctx& x, const StepArgs& a, int b) {
  const TdDevCfg& C = x.C;
  if (x.lane < 24) {
    int64_t v = a.atk_act[(size_t)b * 24 + x.lane];
    const bool bad = v < 0 || v > 4;
    S.atk[x.lane] = bad ? 4 : (int)v;
    S.real_atk[x.lane] = bad ? 4 : (int)v;
  }
  if (x.lane < 4) S.fail_atk[x.lane] = -1;
  {
    bool bad = false;
    if (x.lane < 24) { int64_t v = a.atk_act[(size_t)b * 24 + x.lane]; bad = v < 0 || v > 4; }
    if (ballot(bad)) u.flags |= FLAG_BAD_ACTION;
  }
  wsync();
  if (u.atk_cd != 0) return;
  for (int i = 0; i < u.num_roads; ++i) {
    uint32_t cl = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) cl |= (uint32_t)S.atk[8 * i + k] << (4 * k);
    const bool all4 = cl == 0x44444444u;
    uint32_t real = cl;
    if (MODE == MODE_2P && a.multi) {  // TDMulti multi: every road, always truthy (:201-206)
      summon_cluster(S, u, x, cl, i, &real);
      u.atk_cd = C.atk_interval;
    } else if (all4) {
      if (x.lane == 0) S.fail_atk[i] = 0;               // TDAttack.py:40-42, TDMulti.py:234-236
    } else {
      const int fc = summon_cluster(S, u, x, cl, i, &real);
      if (MODE == MODE_ATK) {
        if (fc == FC_OK) u.atk_cd = C.atk_interval;     // res is a real bool here (TDAttack.py:43-44)
        if (x.lane < 8) S.real_atk[8 * i + x.lane] = (int)((real >> (4 * x.lane)) & 0xfu);
      } else {
        u.atk_cd = C.atk_interval;                      // tuple truthiness (TDMulti.py:237-238)
      }
      if (x.lane == 0) S.fail_atk[i] = fc;
    }
    wsync();
  }
}

}  // namespace td
