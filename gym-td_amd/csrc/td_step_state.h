// td_step_state.h -- one board's state on the device, and how it travels.
// What belongs here: the per-board LDS image (Smem), the wave-uniform scalars (U) and the
// per-step context (Ctx, captured); staging of the constant block; the loads that bring a
// board in from its SoA record (Prefetch, load_board), reset_board, and every store that
// writes the board or a step's per-board outputs back (store_*, StepOut).  No game rule and
// no observation code: those read and change this state (td_step_rules.h, td_step_obs.h).
#pragma once
#include "td_board.h"
#include "td_kernels.h"
#include "td_layout.h"
#include "td_wave.h"

namespace td {

// ---------------------------------------------------------------------------
// per-board LDS image
// ---------------------------------------------------------------------------
template <int NC>
struct alignas(16) Smem {
  static_assert(NC % 4 == 0, "cell and tower maps are moved in 16-B / 4-B units");
  uint32_t cell[NC];      // cell words (td_layout.h), + the tower on the cell in bits 10-13 (tw_nib)
  uint8_t grp[4][NC];     // enemy group (head enemy index) per (type, cell), 0xFF none
  union {
    struct {              // load .. march: the enemy list (written back right after the march)
      double eLP[ECAP];
      double eMg[ECAP];
    };
    float gst[ECAP][4];   // stats .. obs: group stats min, max, avg, count/8 by head enemy
  };
  uint32_t eInf[ECAP];
  double tCd[TCAP];
  uint32_t tInf[TCAP];
  union {
    struct {              // actions: the attacker's clusters (TD-atk / TD-2p), written out right after
      int32_t atk[24];
      int32_t real_atk[24];  // info['RealAction'] of the attacker
      int32_t fail_atk[4];   // info['FailCode'] of the attacker (-1 = no entry)
    };
    struct {              // observation
      float chv[48];      // broadcast channel values
      float d9[64];       // channel 9 by distance (road length < 2L <= 64)
    };
  };
  uint32_t early_go;         // td_step_kernel_small2: the binary-plane windows may be written early (kEarlyGo | dirty classes)
  int32_t flags0;            // the board's flags as loaded (store_board: is the header's second half dirty?)
  uint32_t before;           // the board as loaded, for the dirty classes: cost_bits (bits 0-3)
  int32_t before_lp;         // ... and its base_LP
  TdDevCfg cfg;           // constant block, staged once per board: per-lane table lookups hit LDS
};

template <int NC>
__device__ __forceinline__ void set_tower(Smem<NC>& S, int cell, uint32_t nib) {
  S.cell[cell] = (S.cell[cell] & ~kTwBits) | nib;
}

// Stage the constant block into LDS (16 bytes per lane).
template <int NC>
__device__ __forceinline__ void stage_cfg(Smem<NC>& S, const TdDevCfg* g, int l = (int)(threadIdx.x & 63)) {
  static_assert(sizeof(TdDevCfg) % 16 == 0 && sizeof(TdDevCfg) <= 64 * 16, "cfg staging");
  if (l < (int)(sizeof(TdDevCfg) / 16))
    reinterpret_cast<uint4*>(&S.cfg)[l] = reinterpret_cast<const uint4*>(g)[l];
}
// The same in two halves, so that a step kernel issues the board's loads between them:
// staged in one piece, the block's load was waited for (vmcnt(0)) before any of the
// board's loads went out -- one L2 round trip in front of every board's step.
__device__ __forceinline__ uint4 load_cfg(const TdDevCfg* g, int l) {
  return l < (int)(sizeof(TdDevCfg) / 16) ? reinterpret_cast<const uint4*>(g)[l] : uint4{0u, 0u, 0u, 0u};
}
template <int NC>
__device__ __forceinline__ void store_cfg(Smem<NC>& S, uint4 v, int l) {
  if (l < (int)(sizeof(TdDevCfg) / 16)) reinterpret_cast<uint4*>(&S.cfg)[l] = v;
}

// Wave-uniform scalar board state (identical in every lane).
struct U {
  double cost_def, cost_atk, ep_ret, progress;
  double max_cost;  // captured at reset (TDBoard.py:70)
  int steps, base_LP, atk_cd, def_cd, n, nt, num_roads, end_cell, maxdist, flags, episodes;
  int max_base_LP;  // captured at reset (TDBoard.py:72)
  bool cells_dirty;  // map[6] changed (tower built / destroyed) or a new layout: write the cells back
  bool tw_dirty;     // the tower list changed (build / upgrade / destruct, reset): write tw_inf back
  bool en_touch;     // an enemy plane may have changed since the board was loaded (obs_dirty states the rule)
  uint64_t starts;  // start cells of roads 0-2, 16 bits each (a shift, not an indexed field: keeps U in registers)
  __device__ __forceinline__ int start(int road) const { return (int)((starts >> (16 * road)) & 0xffffu); }
  __device__ __forceinline__ void set_starts(uint32_t s0, uint32_t s1, uint32_t s2) {
    starts = (uint64_t)s0 | ((uint64_t)s1 << 16) | ((uint64_t)s2 << 32);
  }
};

struct Ctx {
  const TdDevCfg& C;  // the current constant block (epoch ep), staged in LDS
  int L, NCr, lane;
  const TdDevCfg* tab;  // every epoch's block (HBM)
  int ep;
  uint32_t Lm = side_magic(L);  // div_side's multiplier
  // The equal-type cluster loop of summon_cluster and board_step's empty-list skip are compiled in.
  // A constant where the kernel builds its Ctx (everything is inlined): the two-wave kernels pass
  // false and keep the unrolled cluster and the unconditional kills-to-compaction stretch -- their
  // non-skipping launch at 65,536 boards, bound by its store stream, measured 0.3 % slower with the
  // two (DESIGN section 5 "Uniform words").
  bool short_cuts = true;
};

// A value an enemy or tower captured when it was created or upgraded (TDElements.py:
// 4-43, 45-63, 134-170): from the block of its epoch -- the staged current one, or
// (after a paramConfig) an older block in HBM.
// The two loads are kept apart by an empty asm on the HBM value, waited for inside its
// branch: otherwise the compiler merges them into one FLAT load of a selected pointer,
// which waits with vmcnt(0) and lgkmcnt(0) at every call (16 FLAT loads in the small
// kernel).  Apart: -0.4 to -0.5 % at 32,768-65,536 boards, +-0.5 % below (r05/s26, s27;
// +-0.6 % in round 3, r03/s17).  The older block's address takes a 24-bit multiply
// (ep * sizeof(TdDevCfg) < 2^24); as x.tab[ep] it took a quarter-rate v_mad_u64_u32.
template <class F>
__device__ __forceinline__ double captured(const Ctx& x, int ep, F f) {
  double v = f(x.C);
  if (ep != x.ep) {
    double w = f(*reinterpret_cast<const TdDevCfg*>(reinterpret_cast<const char*>(x.tab) +
                                                    __umul24((uint32_t)ep, (uint32_t)sizeof(TdDevCfg))));
    __asm__ volatile("" : "+v"(w));
    v = w;
  }
  return v;
}

// ---------------------------------------------------------------------------
// board load / reset / store
// ---------------------------------------------------------------------------
// The inputs of one board step, all loads issued before any is waited on.
// Lane l holds enemy slot l (l < PFE), tower slot l (l < PFT), cells l and l + 64, and one word
// of `w`: lanes 0-23 the header, 24-25 the discrete defender action, 26-37 the
// opponent stream's hot record.
struct Prefetch {
  double lp, mg, tcd;
  uint4 c4;  // cells 4 lane .. 4 lane + 3 (board of L*L % 4 == 0), else cells lane and lane + 64 in .x / .y
  uint32_t inf, tinf, w;
};
// PFE / PFT: enemy / tower slots fetched speculatively with the header (template
// arguments below).  The small-batch kernel (latency-bound) takes 16 of each up front;
// the large-batch kernel (HBM-bound) takes none and loads exactly the live slots once
// the header's counts are in (one dependent round trip, hidden by the other waves).
constexpr int PF_ACT = 24, PF_HOT = 26, PF_SMALL = 16, PF_LARGE = 0;
// (Four enemy slots instead of 16 in TD-def, where 0.02 % of bench.py's steady-state boards
// hold more than 4, read the same bytes -- each slot array's first 128-B line is fetched
// whole either way: PMC 1,534 vs 1,535 B read per board -- in the same time, r06/s5.)
static_assert(offsetof(TdHdr, steps) == 24 && offsetof(TdHdr, start_cell) == 56 && offsetof(TdHdr, episodes) == 76 &&
                  offsetof(TdHdr, max_cost) == 80 && offsetof(TdHdr, max_base_LP) == 88,
              "Prefetch header word map");

template <int PFE, int PFT>
__device__ __forceinline__ void prefetch_issue(Prefetch& P, const StepArgs& a, int b, int lane, int ncr,
                                               bool want_act) {
  const size_t eb = (size_t)b * ECAP, tb = (size_t)b * TCAP, cb = (size_t)b * ncr;
  if (lane < PFE) {  // enemy slots beyond PFE load after the header
    P.lp = a.en_lp[eb + lane];
    P.mg = a.en_mg[eb + lane];
    P.inf = a.en_inf[eb + lane];
  }
  if (lane < PFT) {  // tower slots beyond PFT load after the header
    P.tcd = a.tw_cd[tb + lane];
    P.tinf = a.tw_inf[tb + lane];
  }
  if ((ncr & 3) == 0) {
    P.c4 = lane < (ncr >> 2) ? reinterpret_cast<const uint4*>(a.cells + cb)[lane] : uint4{0u, 0u, 0u, 0u};
  } else {  // (assigned whole: member-wise stores kept P.c4 in scratch in the generic-L build)
    P.c4 = uint4{lane < ncr ? a.cells[cb + lane] : 0u, lane + 64 < ncr ? a.cells[cb + lane + 64] : 0u, 0u, 0u};
  }
  const uint32_t* src;
  if (lane < PF_ACT) src = reinterpret_cast<const uint32_t*>(a.hdr + b) + lane;
  else if (lane < PF_HOT) src = want_act ? reinterpret_cast<const uint32_t*>(a.def_act + b) + (lane - PF_ACT) : nullptr;
  else if (lane < PF_HOT + HOT_WORDS) src = a.opp_hot + (size_t)b * HOT_WORDS + (lane - PF_HOT);
  else src = nullptr;
  P.w = src ? *src : 0u;
}

__device__ __forceinline__ uint32_t lane_word(uint32_t v, int l) { return rdl(v, l); }
// The f64 whose low / high words are held by lanes l / l + 1.
__device__ __forceinline__ double lane_f64(uint32_t v, int l) {
  return __hiloint2double((int)lane_word(v, l + 1), (int)lane_word(v, l));
}

// Commit the prefetched inputs of board b into the LDS image and the scalar state.
// PROGRESS: u.progress is computed here (an f64 division sequence).  Only a caller that renders
// the loaded board as it is asks for it (the board copy: channel 13): a step's summons test the
// step count (summon_cluster), and board_step computes the quotient every later reader uses.
template <int NC, int PFE, int PFT, bool PROGRESS = false>
__device__ __forceinline__ void load_board(Smem<NC>& S, U& u, const Ctx& x, const StepArgs& a, int b, const Prefetch& P) {
  const size_t eb = (size_t)b * ECAP, cb = (size_t)b * x.NCr;
  if ((x.NCr & 3) == 0) {
    // 16-B cell loads: the first 256 cells came with the prefetch, the rest (L > 16)
    // are all issued before any is stored to LDS
    const int n4 = x.NCr >> 2;
    const uint4* g4 = reinterpret_cast<const uint4*>(a.cells + cb);
    uint4* s4 = reinterpret_cast<uint4*>(S.cell);
    constexpr int NR = (NC / 4 + 63) / 64 - 1;  // further 16-B loads per lane: 0 (L <= 16) .. 3 (NC = 1024)
    uint4 r[NR > 0 ? NR : 1];
#pragma unroll
    for (int k = 0; k < NR; ++k) {  // every element assigned (clamped index): the array stays in registers
      const int i = 64 * (k + 1) + x.lane;
      r[k] = g4[i < n4 ? i : n4 - 1];
    }
    if (x.lane < n4) s4[x.lane] = P.c4;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const int i = 64 * (k + 1) + x.lane;
      if (i < n4) s4[i] = r[k];
    }
  } else {
    if (x.lane < x.NCr) S.cell[x.lane] = P.c4.x;
    if (x.lane + 64 < x.NCr) S.cell[x.lane + 64] = P.c4.y;
    for (int i = 128 + x.lane; i < x.NCr; i += 64) S.cell[i] = a.cells[cb + i];
  }
  // TdHdr words (td_common.h): 0-5 cost_def, cost_atk, ep_return; 6 steps, 7 base_LP,
  // 8 atk_cd, 9 def_cd, 10 n_en, 11 n_tw, 12 num_roads, 13 end_cell, 14-16 start_cell,
  // 17 maxdist, 18 flags, 19 episodes, 20-21 max_cost, 22 max_base_LP
  u.cost_def = lane_f64(P.w, 0); u.cost_atk = lane_f64(P.w, 2); u.ep_ret = lane_f64(P.w, 4);
  u.steps = (int)lane_word(P.w, 6); u.base_LP = (int)lane_word(P.w, 7);
  u.atk_cd = (int)lane_word(P.w, 8); u.def_cd = (int)lane_word(P.w, 9);
  u.n = (int)lane_word(P.w, 10); u.nt = (int)lane_word(P.w, 11);
  u.num_roads = (int)lane_word(P.w, 12); u.end_cell = (int)lane_word(P.w, 13);
  u.set_starts((int)lane_word(P.w, 14), (int)lane_word(P.w, 15), (int)lane_word(P.w, 16));
  u.maxdist = (int)lane_word(P.w, 17); u.flags = (int)lane_word(P.w, 18); u.episodes = (int)lane_word(P.w, 19);
  if (x.lane == 0) S.flags0 = u.flags;
  u.max_cost = lane_f64(P.w, 20); u.max_base_LP = (int)lane_word(P.w, 22);
  if constexpr (PROGRESS) u.progress = ddiv((double)u.steps, (double)x.C.max_episode_steps);
  else u.progress = __builtin_nan("");  // board_step sets it before any reader; a read before that shows as a NaN
  u.cells_dirty = false;
  u.tw_dirty = false;
  u.en_touch = false;
  if (x.lane < u.n && x.lane < PFE) { S.eLP[x.lane] = P.lp; S.eMg[x.lane] = P.mg; S.eInf[x.lane] = P.inf; }
  for (int i = PFE + x.lane; i < u.n; i += 64) { S.eLP[i] = a.en_lp[eb + i]; S.eMg[i] = a.en_mg[eb + i]; S.eInf[i] = a.en_inf[eb + i]; }
  uint32_t tinf = P.tinf;
  if (x.lane < u.nt) {
    double tcd = P.tcd;
    if (x.lane >= PFT) {
      const size_t tb = (size_t)b * TCAP;
      tcd = a.tw_cd[tb + x.lane];
      tinf = a.tw_inf[tb + x.lane];
    }
    S.tCd[x.lane] = tcd;
    S.tInf[x.lane] = tinf;
  }
  wsync();
  if (x.lane < u.nt)  // (one tower per cell: no two lanes share a word)
    S.cell[tinf & 0xfffu] |= tw_nib((int)((tinf >> 14) & 1u), (int)((tinf >> 12) & 3u));
  wsync();
}

// Fresh board from a layout record (TDGymBasic.reset :43-53, TDBoard.__init__ :14-79).
template <int NC>
__device__ __forceinline__ void reset_board(Smem<NC>& S, U& u, const Ctx& x, const uint32_t* rec) {
  const TdDevCfg& C = x.C;
  // vector loads only (lane-indexed, then readlane): a record handed over by a
  // concurrently running refill must not come through the scalar cache
  const uint32_t hw = rec[x.lane & (LAYOUT_HDR - 1)];
  for (int i = x.lane; i < x.NCr; i += 64) S.cell[i] = rec[LAYOUT_HDR + i];
  u.num_roads = (int)rdl(hw, 1); u.end_cell = (int)rdl(hw, 2); u.maxdist = (int)rdl(hw, 3);
  u.set_starts(rdl(hw, 4), rdl(hw, 5), rdl(hw, 6));
  u.cost_def = C.def_init_cost; u.cost_atk = C.atk_init_cost;
  u.base_LP = C.base_LP; u.steps = 0; u.progress = 0.0;
  u.max_cost = C.max_cost; u.max_base_LP = C.base_LP;  // TDBoard(max_cost, base_LP) from config at reset
  u.atk_cd = 0; u.def_cd = 0; u.n = 0; u.nt = 0; u.ep_ret = 0.0;
  u.cells_dirty = true;
  u.tw_dirty = true;
  u.en_touch = true;
  wsync();
}

// Cell words back to HBM when map[6] changed or a new layout was loaded (before
// pack_obs_cells reuses the LDS copy).
template <int NC>
__device__ __forceinline__ void store_cells(const Smem<NC>& S, const U& u, const Ctx& x, const StepArgs& a, int b) {
  const size_t cb = (size_t)b * x.NCr;
  if (u.cells_dirty)
    for (int i = x.lane; i < x.NCr; i += 64) sst(&a.cells[cb + i], S.cell[i] & ~kTwBits);
}

__device__ __forceinline__ TdHdr hdr_of(const U& u) {
  TdHdr h;
  h.cost_def = u.cost_def; h.cost_atk = u.cost_atk; h.ep_return = u.ep_ret;
  h.steps = u.steps; h.base_LP = u.base_LP; h.atk_cd = u.atk_cd; h.def_cd = u.def_cd;
  h.n_en = u.n; h.n_tw = u.nt; h.num_roads = u.num_roads; h.end_cell = u.end_cell;
  h.start_cell[0] = u.start(0); h.start_cell[1] = u.start(1); h.start_cell[2] = u.start(2);
  h.maxdist = u.maxdist; h.flags = u.flags; h.episodes = u.episodes;
  h.max_cost = u.max_cost; h.max_base_LP = u.max_base_LP; h.format = kHdrFormat;
  return h;
}

// The towers' words (cool-downs every step, the rest only when the list changed).
template <int NC>
__device__ __forceinline__ void store_towers(const Smem<NC>& S, int nt, bool dirty, int lane, const StepArgs& a, int b) {
  const size_t tb = (size_t)b * TCAP;
  if (lane < nt) {
    sst(&a.tw_cd[tb + lane], S.tCd[lane]);
    if (dirty) sst(&a.tw_inf[tb + lane], S.tInf[lane]);
  }
}

// The header's second half (words 12-23: layout, flags, episodes, the captured max_cost /
// max_base_LP) changes only at an episode end, a reset or a new flag: a step that did none
// of these stores the first 48 B only (hdr_hi false; -48 B written per board and step).
template <int NC>
__device__ __forceinline__ void store_board(const Smem<NC>& S, const U& u, const Ctx& x, const StepArgs& a, int b,
                                            bool hdr_hi = true) {
  if (x.lane == 0) {
    static_assert(sizeof(TdHdr) == 6 * 16, "header stored as 6 x 16 B");
    const TdHdr h = hdr_of(u);
    const uint4* src = reinterpret_cast<const uint4*>(&h);
    uint4* dst = reinterpret_cast<uint4*>(a.hdr + b);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    if (hdr_hi) { dst[3] = src[3]; dst[4] = src[4]; dst[5] = src[5]; }
  }
  // cells were written back by store_cells, enemies at the end of board_step
  store_towers(S, u.nt, u.tw_dirty, x.lane, a, b);
}

// The enemy list after board_step, back to HBM (before enemy_stats reuses its LDS).
template <int NC>
__device__ __forceinline__ void store_enemies(const Smem<NC>& S, const U& u, const Ctx& x, const StepArgs& a, int b) {
  const size_t eb = (size_t)b * ECAP;
  for (int i = x.lane; i < u.n; i += 64) {
    sst(&a.en_lp[eb + i], S.eLP[i]);
    sst(&a.en_mg[eb + i], S.eMg[i]);
    sst(&a.en_inf[eb + i], S.eInf[i]);
  }
}

// The per-board outputs of a step (td_step_io) and the board after it: in
// td_step_kernel_small2 the stepping wave hands them to the second wave in LDS, which
// stores them (store_board, store_outputs) while the stepping wave computes the group
// statistics and broadcast channels -- off the board's critical path.
struct alignas(16) StepOut {
  TdHdr hdr;           // the board's header after the step (6 lanes copy it out, 16 B each)
  int32_t nt, tw_dirty;
  double reward, ep_ret;
  int64_t real_def;
  int32_t ep_steps, fail_def;
  uint32_t done, win, allow, cool;
  uint32_t scan_bad;  // second wave, multi-action scan: a flag was not 0 / 1 / 2 (scan_fold)
  uint32_t go;   // second wave: 0 nothing (a board never reset wrote its own outputs), 1 store and write
                 // half of the late windows, 2 store only (an auto-reset board: the stepping wave writes every window)
  uint32_t any;  // the board has enemies (enemy windows read the group statistics)
  uint32_t hdr_hi;  // the header's second half changed (store_board): 6 lanes store it, else 3
  uint32_t dirty;   // the observation's dirty classes (obs_dirty): the late windows the second wave writes
};

__device__ __forceinline__ void store_outputs(const StepArgs& a, int b, double reward, double ep_ret, int64_t real_def,
                                              int32_t ep_steps, int32_t fail_def, bool done, int win, uint32_t allow,
                                              uint32_t cool, int lane) {
  if (lane != 0) return;
  sst(&a.reward[b], reward);
  sst(&a.done[b], (uint8_t)(done ? 1 : 0));
  if (a.win) sst(&a.win[b], (int8_t)win);
  if (a.allow_next) sst(&a.allow_next[b], (uint8_t)allow);
  if (a.cooldowns) sst(&a.cooldowns[b], (uint8_t)cool);
  if (a.fail_def) sst(&a.fail_def[b], fail_def);
  if (a.real_def && !a.multi) sst(&a.real_def[b], real_def);
  if (a.ep_return) sst(&a.ep_return[b], ep_ret);
  if (a.ep_len) sst(&a.ep_len[b], ep_steps);
  if (done && a.last_ep) {  // the board's last finished episode (td_episode_records)
    td_episode_record r;
    r.ret = ep_ret;
    r.length = ep_steps;
    r.win = win;
    a.last_ep[b] = r;
  }
  if (done && a.ep_stats) {  // device-side episode accounting (SURVEY §8(b) td_episode_stats)
    atomicAdd(&a.ep_stats[0], 1.0);
    atomicAdd(&a.ep_stats[1], ep_ret);
  }
}
__device__ __forceinline__ void store_outputs(const StepArgs& a, int b, const StepOut& o, int lane) {
  store_outputs(a, b, o.reward, o.ep_ret, o.real_def, o.ep_steps, o.fail_def, o.done != 0u, (int)(int32_t)o.win, o.allow,
                o.cool, lane);
}

}  // namespace td
