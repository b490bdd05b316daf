// td_step_obs.h -- the observation of one board, from LDS tables to HBM.
// What belongs here: the group statistics and broadcast channels the planes are made of
// (enemy_stats, d9_table, channel_scalars, pack_obs_cells, obs_value), the output formats
// (ObsFmt), the two writers (write_obs per element, write_obs_lines in line-aligned
// windows, by the window tables of td_obs_win.h), the split of the windows between the two
// waves of a board (obs_half, obs_late_half), the dirty classes of a retained observation
// (cost_bits, obs_dirty) and a reset board's first observation (reset_obs).
#pragma once
#include "td_board.h"
#include "td_kernels.h"
#include "td_step_state.h"
#include "td_wave.h"

namespace td {

// enemy_LP planes (TDBoard.py:355-365): per (type, cell) min / max / sum in list
// order / count, all in numpy float32.  The first enemy of each group (its
// "head") walks the list and owns the group's stats.
template <int NC>
__device__ __forceinline__ void enemy_stats(Smem<NC>& S, const U& u, const Ctx& x) {
  const TdDevCfg& C = x.C;
  const int n = u.n;
  if (n == 0) return;  // write_obs emits zero planes without reading grp
  static_assert((4 * NC) % 16 == 0 && offsetof(Smem<NC>, grp) % 16 == 0, "grp cleared in 16-B units");
  for (int i = x.lane; i < 4 * NC / 16; i += 64)
    reinterpret_cast<uint4*>(&S.grp[0][0])[i] = uint4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  uint32_t key[2];
  float r[2] = {0.0f, 0.0f};
  bool val[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    int i = x.lane + 64 * s;
    val[s] = i < n;
    key[s] = 0;
    if (val[s]) {
      uint32_t e = S.eInf[i];
      key[s] = e & 0x3fffu;  // cell | type << 12
      const int t = en_type(e), lv = en_lv(e);
      r[s] = f32(ddiv(S.eLP[i], captured(x, en_ep(e), [&](const TdDevCfg& c) { return c.e_lp[t][lv]; })));  // LP / maxLP (:358)
    }
  }
  float mn[2] = {1.0f, 1.0f}, mx[2] = {0.0f, 0.0f}, sm[2] = {0.0f, 0.0f};
  int cnt[2] = {0, 0};
  bool head[2] = {val[0], val[1]};
  for (int j = 0; j < n; ++j) {  // enemy j's group key and ratio from the lane that holds it
    const uint32_t kj = j < 64 ? rdl(key[0], j) : rdl(key[1], j - 64);
    const float rj = j < 64 ? rdl(r[0], j) : rdl(r[1], j - 64);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      int i = x.lane + 64 * s;
      if (val[s] && kj == key[s]) {
        if (j < i) head[s] = false;
        else {
          mn[s] = rj < mn[s] ? rj : mn[s];
          mx[s] = rj > mx[s] ? rj : mx[s];
          sm[s] = __fadd_rn(sm[s], rj);
          cnt[s] += 1;
        }
      }
    }
  }
  const float mcl = (float)C.max_cluster_length;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    int i = x.lane + 64 * s;
    if (head[s]) {
      S.gst[i][0] = mn[s];
      S.gst[i][1] = mx[s];
      S.gst[i][2] = __fdiv_rn(sm[s], (float)cnt[s]);
      S.gst[i][3] = __fdiv_rn((float)cnt[s], mcl);
      S.grp[key[s] >> 12][key[s] & 0xfffu] = (uint8_t)i;
    }
  }
  wsync();
}

// Channel 9 by distance (per episode): s[9] = map[4] / (max(map[4]) + 1), an
// int32 scalar divisor promotes to f64, rounded once to f32 (TDBoard.py:121).
template <int NC>
__device__ __forceinline__ void d9_table(Smem<NC>& S, int maxdist, int lane) {
  if (lane <= maxdist) S.d9[lane] = f32(ddiv((double)lane, (double)(maxdist + 1)));
}

// Broadcast channels and the channel-9 table (TDBoard.py:115-142).  Lane l holds channel
// l.  One division sequence per dependency level: every lane picks its own channel's
// operands (1 / 1 where the channel has no quotient) and the wave divides once -- channels
// 5, 11, 12 and the first quotient of 41-44 -- then the four lanes of 41-44 divide by
// max_cluster_length.  (A branch per channel ran five sequences one after another; the
// retained step is bound by the vector unit, where a sequence costs the same for one lane
// as for 64.  While the step was bound by its 18-KB store stream the two forms measured
// 219 vs 214 us at 65,536 boards, profiles/r03/s24.)  Each quotient is one correctly-rounded
// f64 division, rounded once to f32, as before.
// need: the channels the board's written windows read (ObsWinTab::ntab, obs_need): the
// channel-9 table is built only when channel 9 is among them -- a new episode, a step that
// may not skip, and one line misalignment in eight.
template <int NC>
__device__ __forceinline__ void channel_scalars(Smem<NC>& S, const U& u, const Ctx& x, uint64_t need = kChAll) {
  const TdDevCfg& C = x.C;
  const int l = x.lane;
  if (l < 48) {
    const bool is5 = l == 5, isq = l >= 41 && l < 45;
    const bool isdiv = is5 || l == 11 || l == 12 || isq;
    double num = l == 12 ? u.cost_atk : u.cost_def, den = u.max_cost;
    if (is5) { num = (double)u.base_LP; den = (double)u.max_base_LP; }
    if (isq) den = C.e_cost[l - 41][0];
    if (!isdiv) { num = 1.0; den = 1.0; }
    double q = ddiv(num, den);
    if (isq) q = ddiv(q, (double)C.max_cluster_length);
    float v = 0.0f;
    if (isdiv) v = f32(q);
    else if (l == 13) v = f32(u.progress);
    else if (l >= 21 && l < 25) v = (u.cost_def >= C.t_price[l - 21][0]) ? 1.0f : 0.0f;
    S.chv[l] = v;
  }
  if ((need >> 9) & 1ull) d9_table(S, u.maxdist, l);  // wave-uniform
  wsync();
}


// Once the step's actions are done (the towers and map[6] are final), the cell words
// are replaced in LDS by what the rest of the step reads of a cell: the binary
// observation bits (cell_bits, bits 0-20), the march direction map[5] (bits 21-22)
// and the distance to the end map[4] (bits 24-31; channel 9 and the sort key).  The
// board's own cell words must have been written back first (store_cells).
template <int NC>
__device__ __forceinline__ void pack_obs_cells(Smem<NC>& S, const Ctx& x) {
  for (int i = x.lane; i < x.NCr; i += 64) {
    const uint32_t w = S.cell[i];
    S.cell[i] = cell_bits(w, twr_of(w)) | ((uint32_t)cw_dir(w) << 21) | ((uint32_t)cw_dist(w) << 24);
  }
  wsync();
}

template <int NC>
__device__ __forceinline__ float obs_value(const Smem<NC>& S, int ch, int cell, bool any_enemy) {
  const uint32_t w = S.cell[cell];  // packed by pack_obs_cells
  switch (obs_kind(ch)) {
    case OK_BIN: return bitf(w, ch);
    case OK_D9: return S.d9[w >> 24];
    case OK_ENEMY: {
      if (!any_enemy) return 0.0f;
      const int e = ch - 25;
      const uint32_t g = S.grp[e & 3][cell];
      return g == 0xFFu ? 0.0f : S.gst[g][e >> 2];
    }
    default: return S.chv[ch];
  }
}

// Observation stores are non-temporal: 1.2 GB per launch written once and never
// read back by the kernel; as plain stores the dirty lines fill the XCD L2s and
// every state load behind them waits on a write-back (measured: 16 % slower).
__device__ __forceinline__ void obs_store(f32x4* p, f32x4 v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void obs_store(u32x2* p, u32x2 v) { __builtin_nontemporal_store(v, p); }
// The two lines a board shares with its neighbours (written half by this wave, half
// by a wave on another XCD) are stored write-through (sc1) instead: two non-temporal
// partial writes of one line cost ~7 % of the whole stream (scripts/storepol.hip:
// 234 us with nt partial lines, 218 us with sc1 ones = the whole-lines-only bound).
__device__ __forceinline__ void obs_store_shared(__amdgpu_buffer_rsrc_t r, int off, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, off, 0, 16);  // aux 16 = sc1
}
__device__ __forceinline__ void obs_store_shared(__amdgpu_buffer_rsrc_t r, int off, u32x2 v) {
  __builtin_amdgcn_raw_buffer_store_b64(v, r, off, 0, 16);
}

// Buffer store of one unit; AUX: 0 plain, 2 non-temporal, 16 write-through (sc1).  A lane
// whose offset lies beyond the resource's range is dropped by the hardware.
template <int AUX>
__device__ __forceinline__ void obs_buf_store(f32x4 v, __amdgpu_buffer_rsrc_t r, uint32_t off) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, off, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void obs_buf_store(u32x2 v, __amdgpu_buffer_rsrc_t r, uint32_t off) {
  __builtin_amdgcn_raw_buffer_store_b64(v, r, off, 0, AUX);
}

// The observation's output element (td_set_obs_format): float, or _Float16 -- the same
// float32 value, rounded to nearest-even by the last conversion (the _Float16 cast:
// v_cvt_f16_f32 or gfx950's v_cvt_pk_f16_f32, both under the default rounding mode; never
// v_cvt_pkrtz_f16_f32, which rounds toward zero).  One unit
// of the writers below is a quad of 4 cells of one plane in either format: 16 B of
// float32, 8 B of float16, so a 128-B line holds 8 or 16 units.
template <class OT>
struct ObsFmt;
template <>
struct ObsFmt<float> {
  typedef f32x4 Unit;
  static constexpr int UB = 16, UPL = 8;  // bytes per unit, units per 128-B line
  static __device__ __forceinline__ Unit pack(float a, float b, float c, float d) { return f32x4{a, b, c, d}; }
};
template <>
struct ObsFmt<_Float16> {
  typedef u32x2 Unit;
  static constexpr int UB = 8, UPL = 16;
  static __device__ __forceinline__ Unit pack(float a, float b, float c, float d) {
    return __builtin_bit_cast(u32x2, f16x4{(_Float16)a, (_Float16)b, (_Float16)c, (_Float16)d});
  }
};

// The (45, L, L) float32 observation of one board.  The wave writes the batch's
// observation stream in 128-B-aligned 1-KB windows: store k covers the 16-B units
// [A + 64k, A + 64k + 64) of the stream, A = the board's first unit rounded down to
// a 128-B line, and lanes outside the board are masked off.  Every line is then
// written whole by one instruction except the two the board shares with its
// neighbours (a board is 18,000 B at L = 10, not a multiple of 128).  Non-temporal
// stores of partial lines run at ~0.85x the rate of whole ones
// (scripts/membench.hip: 4.3 vs 5.0-5.1 TB/s), so the channel-major walk of the
// planes (800-B runs per store) is not line-aligned enough.  Lane unit i of the board
// is channel i / Q, quad i % Q (Q = L*L/4 quads of 4 cells per plane).
template <int NC, int LT, class OT = float>
__device__ __forceinline__ void write_obs(const Smem<NC>& S, const Ctx& x, OT* out, bool any_enemy) {
  typedef ObsFmt<OT> F;
  typedef typename F::Unit Unit;
  constexpr int UB = F::UB, UPL = F::UPL;
  const int ncr = LT ? LT * LT : x.NCr;
  if ((ncr & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & (UB - 1)) == 0) {  // else: caller buffer not unit-aligned
    const int Q = ncr / 4, n4 = NCH * Q;
    Unit* o4 = reinterpret_cast<Unit*>(out);
    const int mis = (int)((reinterpret_cast<uintptr_t>(o4) / UB) & (UPL - 1));  // units of the line before the board
    // units [0, head) and [tail, n4) lie in lines shared with the neighbouring boards
    const int head = mis ? UPL - mis : 0, tail = ((n4 + mis) & ~(UPL - 1)) - mis;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(o4, 0, n4 * UB, 0x00020000);
    const uint4* cell4 = reinterpret_cast<const uint4*>(S.cell);
    for (int i = x.lane - mis; i < n4; i += 64) {
      if (i < 0) continue;
      const int ch = i / Q, q = i - ch * Q;
      const int kind = obs_kind(ch);
      Unit v;
      if (kind == OK_BIN) {
        const uint4 w = cell4[q];
        const uint32_t c = (uint32_t)ch;
        v = F::pack((float)((w.x >> c) & 1u), (float)((w.y >> c) & 1u), (float)((w.z >> c) & 1u),
                    (float)((w.w >> c) & 1u));
      } else if (kind == OK_CONST) {
        const float c = S.chv[ch];
        v = F::pack(c, c, c, c);
      } else if (kind == OK_D9) {
        const uint4 w = cell4[q];
        v = F::pack(S.d9[w.x >> 24], S.d9[w.y >> 24], S.d9[w.z >> 24], S.d9[w.w >> 24]);
      } else if (any_enemy) {  // wave-uniform
        const int e = ch - 25, st = e >> 2, t = e & 3;
        const uint32_t g4 = *reinterpret_cast<const uint32_t*>(&S.grp[t][4 * q]);
        const uint32_t g0 = g4 & 0xffu, g1 = (g4 >> 8) & 0xffu, g2 = (g4 >> 16) & 0xffu, g3 = g4 >> 24;
        // branch-free: read a clamped slot, keep it only where the cell has a group
        const float f0 = S.gst[g0 & (ECAP - 1)][st], f1 = S.gst[g1 & (ECAP - 1)][st];
        const float f2 = S.gst[g2 & (ECAP - 1)][st], f3 = S.gst[g3 & (ECAP - 1)][st];
        v = F::pack(g0 != 0xffu ? f0 : 0.0f, g1 != 0xffu ? f1 : 0.0f, g2 != 0xffu ? f2 : 0.0f, g3 != 0xffu ? f3 : 0.0f);
      } else {
        v = F::pack(0.0f, 0.0f, 0.0f, 0.0f);
      }
      if (i < head || i >= tail) obs_store_shared(rs, i * UB, v);
      else obs_store(o4 + i, v);
    }
  } else {
    const int nf = NCH * ncr;
    for (int f = x.lane; f < nf; f += 64) {
      const int ch = f / ncr;
      out[f] = (OT)obs_value(S, ch, f - ch * ncr, any_enemy);
    }
  }
}

// The channels a board's written windows read (see channel_scalars): every channel unless
// the step kept its episode and may skip, then ObsWinTab::ntab by the board's misalignment
// and its dirty classes (wave-uniform).  `out` as write_obs_lines takes it.
template <int LT, class OT>
__device__ __forceinline__ uint64_t obs_need(const OT* out, uint32_t dirty) {
  typedef ObsFmt<OT> F;
  if ((dirty & (OD_STATIC | OD_ALWAYS)) != OD_ALWAYS) return kChAll;
  const int mis = (int)((reinterpret_cast<uintptr_t>(out) / F::UB) & (F::UPL - 1));
  return ObsWinTab<LT, F::UPL>::ntab.w[mis][(__builtin_amdgcn_readfirstlane(dirty) >> 1) & 15u];
}

// The (45, L, L) float32 observation of one board for compile-time L, into a
// 16-B-aligned buffer: the 128-B-aligned 1-KB windows of write_obs (store k covers
// stream units [A + 64k, A + 64k + 64), A = the board's first unit rounded down to a
// line), software-pipelined.  For G windows at a time every lane first issues its
// LDS reads -- the 16-B packed cell quad (at 10x10 not in a window of broadcast channels alone) and
// one word that is the broadcast value (chv) or the enemy group quad (grp) -- then the
// windows are computed and stored.
// The window's channel mix is wave-uniform (SALU): a window of one class takes a
// short path, the per-cell tables (channel 9, enemy stats) are read only where the
// window holds such channels.  Stores are buffer stores whose lanes outside the board
// get an out-of-range offset: the hardware drops them, so no lane is masked off by a
// branch.  wt: every line write-through (sc1) instead of non-temporal, where the
// batch's observation fits the 256-MiB Infinity Cache (scripts/storepol.hip at 8,192
// boards, 147 MB: 21.8 us sc1, 30.0 us nt; at 65,536 boards, 1.18 GB, nt whole lines
// are the fastest form, with the two lines shared with the neighbours sc1).
//
// PASS: 0 every window; 1 only the windows of binary planes alone (ObsWinTab class 0:
// roads, end, starts, buildable, tower level / type -- final once the step's actions
// are, td_step_kernel_small2 writes them early); 2 every other window.
// edge_wt: how the two lines the board shares with its neighbours are stored.  2 (default):
// plain write-back stores -- with the XCD-contiguous board map (StepArgs::xcd_map) the
// neighbours' waves run on this XCD and its L2 merges the two halves into one line write
// (a pair split across two XCDs is written back byte-masked by both L2s); 1: write-through
// (sc1).  2 vs 1 at 65,536 boards: 1.088x vs 1.093x the algorithmic bytes, step time +-0
// (profiles/r04/s20); non-temporal partial lines measured 233 vs 212 us (r04/s4).
//
// OT = _Float16: the same units, windows and classes with 8-B units -- a wave store is
// 512 B, four whole lines; a board starts at one of 16 unit offsets in its line
// (ObsWinTab<LT, 16>) and has one window more where N4 + 15 crosses a multiple of 64.
//
// SKIP (td_retain_obs): `dirty` is the board's set of dirty classes (OD_*, wave-uniform); a
// window none of whose classes is dirty (ObsWinTab::dtab) is left as the last write left
// it -- skipped before its LDS reads are issued, as PASS skips windows.  A window that is
// written is written whole, as without SKIP.
template <int NC, int LT, int KB = 0, int KE = -1, int G = 4, int PASS = 0, class OT = float, bool SKIP = false>
__device__ __forceinline__ void write_obs_lines(const Smem<NC>& S, int lane, OT* out, bool any_enemy, bool wt,
                                                int edge_wt = 1, uint32_t dirty = OD_ALL) {
  static_assert(LT >= 8, "a 128-B line spans at most two channel planes");
  typedef ObsFmt<OT> F;
  constexpr int UB = F::UB, UPL = F::UPL;
  constexpr int Q = LT * LT / 4, N4 = NCH * Q;
  constexpr int K = KE >= 0 ? KE : (N4 + UPL - 1 + 63) / 64;  // windows [KB, K) of the board's (N4 + UPL - 1 + 63) / 64
  constexpr uint32_t OOB = 0x80000000u;  // beyond the buffer's num_records: store dropped
  const char* const sb = reinterpret_cast<const char*>(&S);
  const int o_cell = (int)(reinterpret_cast<const char*>(S.cell) - sb);  // packed cell words (pack_obs_cells)
  const int o_grp = (int)(reinterpret_cast<const char*>(&S.grp[0][0]) - sb);
  const int o_chv = (int)(reinterpret_cast<const char*>(S.chv) - sb);
  const int o_d9 = (int)(reinterpret_cast<const char*>(S.d9) - sb);
  const int o_gst = (int)(reinterpret_cast<const char*>(&S.gst[0][0]) - sb);
  const int mis = (int)((reinterpret_cast<uintptr_t>(out) / UB) & (UPL - 1));  // units of the line before the board
  const int head = mis ? UPL - mis : 0, tail = ((N4 + mis) & ~(UPL - 1)) - mis;  // [0, head), [tail, N4): shared lines
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(out, 0, N4 * UB, 0x00020000);
  const int i0 = lane - mis;
  typedef Div24<Q, N4 + 64> DivQ;  // unit -> channel (every unit read is in [0, N4))
  // the window's channel class and edge bit (wave-uniform, ObsWinTab)
  auto wclass = [&](int k) { return (ObsWinTab<LT, UPL>::tab.w[mis][k >> 3] >> (4 * (k & 7))) & 7u; };
  if (SKIP) dirty = __builtin_amdgcn_readfirstlane(dirty);
  auto wclean = [&](int k) { return SKIP && ((ObsWinTab<LT, UPL>::dtab.w[mis][k >> 2] >> (8 * (k & 3))) & dirty) == 0u; };
  // only a window at either end of the board holds lanes outside it (i < 0, i >= N4):
  // clamp there, so every lane reads LDS inside the board image
  auto unit = [&](int i, uint32_t wc) { return (wc & 4u) ? (i < 0 ? 0 : (i > N4 - 1 ? N4 - 1 : i)) : i; };
  for (int k0 = KB; k0 < K; k0 += G) {
    uint4 A[G];
    uint32_t W[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int k = k0 + j;
      if ((K - KB) % G == 0 || k < K) {
        const uint32_t wc = wclass(k);
        if (PASS != 0 && (((wc & 3u) == 0) != (PASS == 1))) continue;  // wave-uniform
        if (wclean(k)) continue;
        const int i = unit(i0 + 64 * k, wc);
        const int ch = DivQ::div(i), q = i - ch * Q;
        // 10x10: a window of broadcast channels alone reads the channel's value and no cell
        // quad (-50 VALU, -169 SALU per wave of the retained step; at 20x20 and 30x30, whose
        // window loop stays rolled, the same skip measured 0.9 and 1.5 % slower)
        if constexpr (LT == 10) {
          if ((wc & 3u) == 1) {
            W[j] = *reinterpret_cast<const uint32_t*>(sb + o_chv + 4 * ch);
            continue;
          }
        }
        A[j] = *reinterpret_cast<const uint4*>(sb + o_cell + 16 * q);
        if ((wc & 3u) == 1) {  // broadcast channels only: the channel's value
          W[j] = *reinterpret_cast<const uint32_t*>(sb + o_chv + 4 * ch);
        } else if ((wc & 3u) >= 2) {
          // enemy plane: the cell quad's group bytes; else the channel's broadcast value
          // (bit select: a ternary here compiled to a divergent branch)
          const int e = ch - 25;
          const int wa = o_grp + (e & 3) * NC + 4 * q, wb = o_chv + 4 * ch, m = -(int)((unsigned)e < 16u);
          const int wo = wb ^ ((wa ^ wb) & m);
          W[j] = *reinterpret_cast<const uint32_t*>(sb + wo);
        } else {
          W[j] = 0u;  // binary planes only: the cell quad is all
        }
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int k = k0 + j;
      if (!((K - KB) % G == 0 || k < K)) continue;
      const uint32_t wc = wclass(k);
      if (PASS != 0 && (((wc & 3u) == 0) != (PASS == 1))) continue;
      if (wclean(k)) continue;
      const bool edge = (wc & 4u) != 0;  // the window holds a line shared with a neighbour
      const int i = i0 + 64 * k;
      const int ch = DivQ::div(unit(i, wc));
      const int e = ch - 25;
      const bool isen = (unsigned)e < 16u, isd9 = ch == 9, isbin = ((kChBin >> ch) & 1ull) != 0;
      const uint32_t a4[4] = {A[j].x, A[j].y, A[j].z, A[j].w};
      float v[4];
      if ((wc & 3u) == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (float)((a4[c] >> ch) & 1u);
      } else if ((wc & 3u) == 1) {
        const float cv = __uint_as_float(W[j]);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = cv;
      } else if ((wc & 3u) == 2 && !any_enemy) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = 0.0f;
      } else {
        // a window of several channel kinds: each lane takes its own channel's path
        // (a select over every kind's value measured 1.5 % slower at 8,192 boards)
        if (isbin) {
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = (float)((a4[c] >> (ch & 31)) & 1u);
        } else if (isd9) {  // channel 9 by distance
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = *reinterpret_cast<const float*>(sb + o_d9 + 4 * (int)(a4[c] >> 24));
        } else if (isen && any_enemy) {  // enemy stats by the cell's group head
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const uint32_t g = (W[j] >> (8 * c)) & 0xffu;
            const float f = *reinterpret_cast<const float*>(sb + o_gst + 16 * (int)(g & 0x7fu) + 4 * ((e >> 2) & 3));
            v[c] = g != 0xffu ? f : 0.0f;
          }
        } else {
          const float cv = isen ? 0.0f : __uint_as_float(W[j]);
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = cv;
        }
      }
      const auto val = F::pack(v[0], v[1], v[2], v[3]);
      const uint32_t off = (uint32_t)i * (uint32_t)UB;  // i < 0 or i >= N4: out of range already
      if (wt) {  // wave-uniform
        obs_buf_store<16 /* sc1 */>(val, rs, off);
      } else if (!edge) {  // whole lines of this board only
        obs_buf_store<2 /* nt */>(val, rs, off);
      } else {
        const bool shared = i < head || i >= tail;  // a line shared with a neighbouring board
        obs_buf_store<2 /* nt */>(val, rs, shared ? OOB : off);
        if (edge_wt == 2)
          obs_buf_store<0 /* plain */>(val, rs, shared ? off : OOB);
        else
          obs_buf_store<16 /* sc1 */>(val, rs, shared ? off : OOB);
      }
    }
  }
}

// Observation windows written by the stepping wave of a two-wave board (the first half).
template <int LT>
__host__ __device__ constexpr int obs_half() { return ((NCH * LT * LT / 4 + 7 + 63) / 64 + 1) / 2; }
// After the second wave's early pass over the binary-plane windows: the first window of
// the second wave's share of the rest, so both waves write half of the remaining
// windows (counted at a line-aligned board; ObsWinTab class != 0).
template <int LT, class OT = float>
constexpr int obs_late_half() {
  typedef ObsWinTab<LT, ObsFmt<OT>::UPL> Tab;
  constexpr int K = Tab::K;
  int late = 0;
  for (int k = 0; k < K; ++k) late += (Tab::cls(0, k) & 3u) != 0u;
  int seen = 0;
  for (int k = 0; k < K; ++k) {
    if (2 * seen >= late) return k;
    seen += (Tab::cls(0, k) & 3u) != 0u;
  }
  return K;
}

// The four bits of channels 21-24 (channel_scalars): cost_def reaches tower t's cost.
__device__ __forceinline__ uint32_t cost_bits(double cost_def, const TdDevCfg& C) {
  uint32_t m = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) m |= (cost_def >= C.t_price[t][0]) ? (1u << t) : 0u;
  return m;
}

// The dirty classes of a board's observation after its step (td_retain_obs), against the
// board as loaded (Smem::before, before_lp).  Every class unless the step may skip
// (StepArgs::obs_skip) and the board kept its episode: a new episode has a new layout.
// tw_dirty: the tower list changed (it decides the tower-word stores too).
// The enemy planes hold, per (type, cell), the minimum, maximum and mean (summed in list
// order) of LP / max LP and count / max_cluster_length.  They are dirty only when the step
// touched one of those (U::en_touch): an enemy was summoned (summon_cluster), the stable sort
// moved one, a tower's shot landed, or an enemy entered a new cell (board_step) -- a kill
// implies a shot, a leak a move.  The slow-down counter, the margin and the cool-downs are not
// in the observation; max_cluster_length and an enemy's captured max LP change only with the
// config, and a config change forces a launch that may not skip (td_obs_ledger.h).  A board
// whose enemy stands in its cell unshot keeps its 16 planes as they are.
template <int NC>
__device__ __forceinline__ uint32_t obs_dirty(const Smem<NC>& S, const U& u, const TdDevCfg& C, bool skip, bool was_reset) {
  if (!skip || was_reset) return OD_ALL;
  const uint32_t bf = S.before;
  return OD_ALWAYS | (u.tw_dirty ? OD_TOWER : 0u) | (u.base_LP != S.before_lp ? OD_LP : 0u) |
         (cost_bits(u.cost_def, C) != (bf & 15u) ? OD_COST : 0u) | (u.en_touch ? OD_ENEMY : 0u);
}
constexpr uint32_t kEarlyGo = 0x80000000u;  // Smem::early_go: the second wave's early pass may run (| its dirty classes)

// The first observation of a board just reset (no enemies yet).
template <int NC, int LT, class OT>
__device__ __forceinline__ void reset_obs(const Smem<NC>& S, const Ctx& x, const StepArgs& a, int b) {
  OT* const o = reinterpret_cast<OT*>(a.obs) + (size_t)b * NCH * x.NCr;
  if constexpr (LT != 0) {
    if ((reinterpret_cast<uintptr_t>(a.obs) & (ObsFmt<OT>::UB - 1)) == 0)
      write_obs_lines<NC, LT, 0, -1, 4, 0, OT>(S, x.lane, o, false, false);
    else write_obs<NC, LT, OT>(S, x, o, false);
  } else {
    write_obs<NC, LT, OT>(S, x, o, false);
  }
}

}  // namespace td
