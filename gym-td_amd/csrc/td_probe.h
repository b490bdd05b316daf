// td_probe.h -- probes (td_probe, td_probe_boards[_dev]): `reps` independent random playouts of
// every board served, in ONE launch, from the board's present state, which is only read.  Replica
// r of board b is td_playout_boards' playout of that board at ticket + r * steps, its effects on
// the handle discarded: the sub-steps are playout_board's own text (td_playout.h, PROBE), which
// ends after its loop with the outputs and stores nothing else.
//
//   load               the board once, as a playout loads it
//   the stream         TD-def / TD-atk: the built-in opponent draws from the board's CPython
//                      stream, which twists lazily IN PLACE (WaveMt: w[q] = y).  A probe may not
//                      write those words, and the replicas of one board would race on them.  So
//                      each wave copies the board's 624 words into LDS (2,496 B) and runs its
//                      WaveMt there, seeded from the hot record as the playout's: lazy twists,
//                      block wraps and refills of the pre-drawn window all land in the copy.
//                      Every replica of a board starts from the same stream position; they
//                      differ through the sampled side only.  TD-2p has no built-in opponent
//                      and takes no copy.
//   outputs            row b * reps + r of the caller's [B][reps] buffers: reward, done, win,
//                      steps_run, first_def, first_atk -- and not one byte else
//
// What belongs here: the kernels' body.  The kernels and their rows are td_probe.hip's.
#pragma once
#include "td_playout.h"

namespace td {

// One wave per (entry, replica), one board image per workgroup, the grid n * reps.  The
// XCD-contiguous map is applied to the (entry, replica) index k = entry * reps + replica:
// consecutive k run on one XCD, so the replicas of a board load its state lines through one L2.
// The entries are q.p.ids[0 .. n) with n as td_list_dev.h makes it, or every board.
template <int LT, int MODE>
__device__ __forceinline__ void probe_kernel_body(const StepArgs& a, const ProbeArgs& q) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  constexpr int MT2 = MT_N / 2;  // the stream as 8-B words (a board's record is 8-B aligned)
  static_assert(MT_N % 2 == 0 && (OPP_WORDS * sizeof(uint32_t)) % sizeof(uint2) == 0, "8-B loads of the stream");
  __shared__ Smem<NC> S;
  __shared__ uint32_t raw[NC];  // the raw cell words (playout_board)
  __shared__ uint2 mt[MODE == MODE_2P ? 1 : MT2];  // this replica's copy of the opponent's stream
  const int i = (int)blockIdx.x;
  prologue_args(a);
  const int n = q.p.ids ? list_length(q.p.cap, q.p.count, q.p.verdict) : a.B;
  const int waves = n * q.reps;  // (the launch refused a grid past 2^31 - 1)
  if (i >= waves) return;
  const uint32_t k = (uint32_t)(a.xcd_map ? xcd_board(i, waves) : i);
  const int e = (int)(k / (uint32_t)q.reps), r = (int)(k - (uint32_t)e * (uint32_t)q.reps);
  const int b = q.p.ids ? list_word(q.p.ids, e) : e;
  const int L = LT ? LT : a.L;
  const Ctx x{S.cfg, L, L * L, (int)(threadIdx.x & 63), a.cfgs, a.epoch};
  const uint4 cfgv = load_cfg(a.cfg, x.lane);
  Prefetch P;
  prefetch_issue<PF_LARGE, PF_LARGE>(P, a, b, x.lane, x.NCr, false);
  if constexpr (MODE != MODE_2P) {
    // the stream's loads behind the board's, all issued before any is stored
    const uint2* g = reinterpret_cast<const uint2*>(a.opp_mt + (size_t)b * OPP_WORDS);
    constexpr int NR = (MT2 + 63) / 64;
    uint2 v[NR];
#pragma unroll
    for (int t = 0; t < NR; ++t) {  // every element assigned (clamped index): the array stays in registers
      const int w = 64 * t + x.lane;
      v[t] = g[w < MT2 ? w : MT2 - 1];
    }
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      const int w = 64 * t + x.lane;
      if (w < MT2) mt[w] = v[t];
    }
  }
  store_cfg(S, cfgv, x.lane);
  wsync();
  PlayoutArgs p = q.p;
  p.ticket = q.p.ticket + (uint64_t)(uint32_t)r * (uint64_t)(uint32_t)a.frame_skip;
  playout_board<NC, LT, MODE, true>(S, raw, x, a, p, b, P, reinterpret_cast<uint32_t*>(mt),
                                    (int)((uint32_t)b * (uint32_t)q.reps + (uint32_t)r));
}

}  // namespace td
