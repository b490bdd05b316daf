// td_copy_body.h -- what the two board-copy kernels share: td_copy_kernel (td_copy.hip,
// td_copy_boards) and td_copy_list_kernel (td_copy_list.hip, td_copy_boards_dev).  Device text
// only: the register slices a pair's state travels in, the observation writer, and the body of
// a pair.
//
// The body is a macro, not a function, and each kernel has a unit of its own: the copy kernel
// must stay, instruction for instruction, the code it was (scripts/kernel_isa_digest.py), and
// either a function boundary around the body (forced inline, with the LDS object inside or
// handed in) or a second kernel beside it in the unit changed how the compiler forms a few LDS
// addresses in it -- one to three instructions, measured with that script.  As a macro the
// kernel's token stream is what it was; the list kernel expands the same text with its own two
// id expressions.
#pragma once
#include "td_kernels.h"
#include "td_step_launch.h"
#include "td_step_obs.h"
#include "td_step_state.h"

namespace td {


// Up to PER * 64 words of T (16 B, or 8 B) of one per-board slice, a word per lane and round,
// held in registers between its loads and its stores: the kernel issues the loads of every
// slice before the first store, so a pair's state costs two memory round trips (the header,
// whose counts bound the slices, then everything else), not one per slice.  src and dst are
// aligned to T; lanes past `units` load a clamped index and store nothing.
template <int PER, class T = uint4>
struct Slice {
  T r[PER];
  __device__ __forceinline__ void load(const void* src, int units, int lane) {
    const T* s = reinterpret_cast<const T*>(src);
    if (units <= 0) return;  // wave-uniform
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = 64 * k + lane;
      r[k] = s[i < units ? i : units - 1];
    }
  }
  __device__ __forceinline__ void store(void* dst, int units, int lane) const {
    T* d = reinterpret_cast<T*>(dst);
    if (units <= 0) return;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = 64 * k + lane;
      if (i < units) sst(&d[i], r[k]);
    }
  }
};

// One MT19937 record (OPP_WORDS = 626 words, 2,504 B: the record of an even board starts on a
// 16-B boundary, that of an odd board 8 B past one).  Boards of the same parity: 156 aligned
// 16-B words and the 8 B left over in front of them or behind; else 313 8-B words.
struct MtCopy {
  static_assert(OPP_WORDS % 4 == 2, "an MT record is 16-B words and one 8-B word");
  Slice<(OPP_WORDS / 4 + 63) / 64> q;
  Slice<(OPP_WORDS / 2 + 63) / 64, uint2> d;
  uint2 rest;
  int lead;  // -1: 8-B words; else the 16-B words start `lead` (0 or 2) words into the record
  __device__ __forceinline__ void load(const uint32_t* src, const uint32_t* dst, int lane) {
    if (((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15u) != 0) {  // wave-uniform
      lead = -1;
      d.load(src, OPP_WORDS / 2, lane);
    } else {
      lead = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
      if (lane == 0) rest = *reinterpret_cast<const uint2*>(src + (lead ? 0 : OPP_WORDS - 2));
      q.load(src + lead, OPP_WORDS / 4, lane);
    }
  }
  __device__ __forceinline__ void store(uint32_t* dst, int lane) const {
    if (lead < 0) {
      d.store(dst, OPP_WORDS / 2, lane);
    } else {
      if (lane == 0) sst(reinterpret_cast<uint2*>(dst + (lead ? 0 : OPP_WORDS - 2)), rest);
      q.store(dst + lead, OPP_WORDS / 4, lane);
    }
  }
};

// The destination's whole observation row from the staged source board.
template <int NC, int LT, class OT>
__device__ __forceinline__ void copy_obs(const Smem<NC>& S, const U& u, const Ctx& x, const StepArgs& a, int db) {
  OT* const o = reinterpret_cast<OT*>(a.obs) + (size_t)db * NCH * x.NCr;
  // the handle's store policy for rows written between steps: whole lines non-temporal, the
  // two lines shared with the neighbouring boards as a.edge_wt says (their halves survive)
  if constexpr (LT != 0) {
    if ((reinterpret_cast<uintptr_t>(a.obs) & (ObsFmt<OT>::UB - 1)) == 0)
      write_obs_lines<NC, LT, 0, -1, 4, 0, OT>(S, x.lane, o, u.n > 0, false, a.edge_wt);
    else write_obs<NC, LT, OT>(S, x, o, u.n > 0);
  } else {
    write_obs<NC, LT, OT>(S, x, o, u.n > 0);
  }
}

// One pair of a copy of n pairs, in a kernel that has StepArgs a, the pair count n (blocks at or
// past it exit at once), LT / NC and __shared__ Smem<NC> S in scope.  SRC_AT / DST_AT:
// expressions in `i` (the pair this block serves) for the source's and the destination's id;
// the ids are validated before the kernel runs: every one in [0, B), no destination named
// twice, none that is also a source.
#define TD_COPY_PAIR_BODY(SRC_AT, DST_AT) \
  const int blk = (int)blockIdx.x;                                                                                       \
  if (blk >= n) return;                                                                                                  \
/* consecutive pairs on one XCD, as the step places consecutive boards: the lines two */                                 \
/* neighbouring destination rows share are merged in that XCD's L2 */                                                    \
  const int i = a.xcd_map ? xcd_board(blk, n) : blk;                                                                     \
  const int sb = (SRC_AT), db = (DST_AT);                                                                                \
  const int lane = (int)threadIdx.x;                                                                                     \
  const int L = LT ? LT : a.L, ncr = L * L;                                                                              \
                                                                                                                         \
/* ---- state: the header first (its counts bound the slot slices), then every slice's loads, */                         \
/* then every store */                                                                                                   \
  static_assert(sizeof(TdHdr) == 6 * 16 && offsetof(TdHdr, n_en) == 40 && offsetof(TdHdr, n_tw) == 44, "header words");  \
  const uint4 h4 = reinterpret_cast<const uint4*>(a.hdr + sb)[lane < 6 ? lane : 5];                                      \
  int ne = (int)rdl(h4.z, 2), nt = (int)rdl(h4.w, 2);                                                                    \
  ne = ne < 0 ? 0 : (ne > ECAP ? ECAP : ne);                                                                             \
  nt = nt < 0 ? 0 : (nt > TCAP ? TCAP : nt);                                                                             \
  const size_t se = (size_t)sb * ECAP, de = (size_t)db * ECAP, st = (size_t)sb * TCAP, dt = (size_t)db * TCAP;           \
  const uint32_t* sc = a.cells + (size_t)sb * ncr;                                                                       \
  uint32_t* dc = a.cells + (size_t)db * ncr;                                                                             \
  const bool quads = (ncr & 3) == 0;  /* (a board's cell words are 16-B aligned only where L * L % 4 == 0) */            \
  static_assert(ECAP / 2 <= 64 && HOT_WORDS % 4 == 0, "one 16-B word per lane; hot record in 16-B words");               \
  Slice<1> lp, mg, einf, tcd, tinf, hot;                                                                                 \
  Slice<(NC / 4 + 63) / 64> cells;                                                                                       \
  MtCopy mt;                                                                                                             \
  lp.load(a.en_lp + se, (ne + 1) / 2, lane);                                                                             \
  mg.load(a.en_mg + se, (ne + 1) / 2, lane);                                                                             \
  einf.load(a.en_inf + se, (ne + 3) / 4, lane);                                                                          \
  tcd.load(a.tw_cd + st, (nt + 1) / 2, lane);                                                                            \
  tinf.load(a.tw_inf + st, (nt + 3) / 4, lane);                                                                          \
  if (quads) cells.load(sc, ncr / 4, lane);                                                                              \
  mt.load(a.opp_mt + (size_t)sb * OPP_WORDS, a.opp_mt + (size_t)db * OPP_WORDS, lane);                                   \
  hot.load(a.opp_hot + (size_t)sb * HOT_WORDS, HOT_WORDS / 4, lane);                                                     \
  if (lane < 6) sst(reinterpret_cast<uint4*>(a.hdr + db) + lane, h4);                                                    \
  lp.store(a.en_lp + de, (ne + 1) / 2, lane);                                                                            \
  mg.store(a.en_mg + de, (ne + 1) / 2, lane);                                                                            \
  einf.store(a.en_inf + de, (ne + 3) / 4, lane);                                                                         \
  tcd.store(a.tw_cd + dt, (nt + 1) / 2, lane);                                                                           \
  tinf.store(a.tw_inf + dt, (nt + 3) / 4, lane);                                                                         \
  if (quads) cells.store(dc, ncr / 4, lane);                                                                             \
  else                                                                                                                   \
    for (int k = lane; k < ncr; k += 64) sst(&dc[k], sc[k]);                                                             \
  mt.store(a.opp_mt + (size_t)db * OPP_WORDS, lane);                                                                     \
  hot.store(a.opp_hot + (size_t)db * HOT_WORDS, HOT_WORDS / 4, lane);                                                    \
/* random_agent=False: the numpy stream is the opponent's too, and nothing is staged ahead of */                         \
/* it.  (random_agent=True: the destination keeps its own layout stream, ring and claim.) */                             \
  if (a.opp_np) {                                                                                                        \
    mt.load(a.np_mt + (size_t)sb * OPP_WORDS, a.np_mt + (size_t)db * OPP_WORDS, lane);                                   \
    mt.store(a.np_mt + (size_t)db * OPP_WORDS, lane);                                                                    \
  }                                                                                                                      \
                                                                                                                         \
/* ---- observation: what a full write of the source's state leaves */                                                   \
  if (!a.obs) return;                                                                                                    \
  const int nr = (int)rdl(h4.x, 3);                                                                                      \
  if (nr < 1 || nr > 3) return;  /* no episode: the row is left as it is (as td_reset leaves a failed draw's) */         \
  stage_cfg(S, a.cfg);                                                                                                   \
  const Ctx x{S.cfg, L, ncr, lane, a.cfgs, a.epoch};                                                                     \
  Prefetch P;                                                                                                            \
  prefetch_issue<PF_SMALL, PF_SMALL>(P, a, sb, lane, ncr, false);                                                        \
  U u;                                                                                                                   \
  load_board<NC, PF_SMALL, PF_SMALL, true>(S, u, x, a, sb, P);                                                           \
  enemy_stats(S, u, x);                                                                                                  \
  channel_scalars(S, u, x);                                                                                              \
  pack_obs_cells(S, x);                                                                                                  \
  if (a.obs_f16) copy_obs<NC, LT, _Float16>(S, u, x, a, db);                                                             \
  else copy_obs<NC, LT, float>(S, u, x, a, db);

}  // namespace td
