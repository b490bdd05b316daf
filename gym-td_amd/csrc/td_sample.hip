// td_sample.hip -- td_sample_kernel: one uniformly drawn legal action per side and board
// (td_sample_actions, td_sample_actions_boards, td_sample_actions_boards_dev), by td_sample.h's
// rule over td_mask.h's verdicts.
//
// Shape: td_mask_list_kernel's -- one wave per entry, kSampleWaves entries per workgroup under
// the XCD-contiguous group map, each wave with an LDS row of its own that only wsync() orders,
// count and verdict as wave-uniform loads through the constant address space.  ids == nullptr
// serves every board: entry i is board i.
//
// Per board the wave puts the row of fail codes together in LDS as mask_board does
// (td_mask_body.h: header words, cell words, tower lanes; that text is repeated here, so the
// mask kernels compile to the code they were) and does not store it.  Lane l owns the P
// consecutive 16-B pieces [l P, (l + 1) P) of the row, P = ceil(pieces / 64): it counts their
// legal bytes (mask_legal4 and one population count per piece), a wave prefix sum over the 64
// counts gives n_def and the one lane whose range holds the k-th candidate, and
// that lane walks its pieces to the byte.  The attacker's 12 verdicts are one ballot.  While
// the defender's cool-down is closed, and on a board that was never reset, nothing is legal:
// the row is not built.
//
// Budget: no scratch; LDS = kSampleWaves * SampleRow<L>::BYTES, a row being the 6 L^2 codes
// rounded up to 16 B (L = 32 for the generic build): 2,432 / 9,600 / 21,632 / 24,576 B at
// L = 10 / 20 / 30 / generic.  The prefix sum runs on lane shuffles and takes no LDS
// (a DPP row scan in its place measured the same: profiles/sample_actions/sample_bench_dpp_scan.jsonl).
#include <cstddef>

#include "td_kernels.h"
#include "td_mask.h"
#include "td_sample.h"
#include "td_wave.h"

namespace td {

namespace {

template <int LT>
struct SampleRow {
  static constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  static constexpr int BYTES = (6 * NC + 15) & ~15;
  static constexpr int PER_LANE = (BYTES / 16 + 63) / 64;  // P
};

// the legal bytes of one 16-B piece, one bit each (byte i of word q: bit 8 i + q -- for counting,
// not in the row's order)
__device__ __forceinline__ uint32_t legal16(const u32x4 x) {
  return mask_legal4(x.x, true) | (mask_legal4(x.y, true) << 1) | (mask_legal4(x.z, true) << 2) |
         (mask_legal4(x.w, true) << 3);
}

// R: the wave's own SampleRow<LT>::BYTES of LDS, 16-B aligned; only wsync() orders its accesses.
template <int LT>
__device__ __forceinline__ void sample_board(const SampleArgs& a, int b, int lane, uint8_t* const R) {
  const int L = LT ? LT : a.L, NC = L * L;
  const TdDevCfg& C = *a.cfg;

  // the header: 24 words, one per lane, then lane broadcasts (as mask_board)
  const uint32_t* const hw = reinterpret_cast<const uint32_t*>(a.hdr + b);
  const uint32_t w = lane < (int)(sizeof(TdHdr) / 4) ? hw[lane] : 0u;
  static_assert(offsetof(TdHdr, cost_def) == 0 && offsetof(TdHdr, cost_atk) == 8 && offsetof(TdHdr, steps) == 24 &&
                offsetof(TdHdr, atk_cd) == 32 && offsetof(TdHdr, def_cd) == 36 && offsetof(TdHdr, n_en) == 40 &&
                offsetof(TdHdr, n_tw) == 44 && offsetof(TdHdr, num_roads) == 48, "TdHdr words read below");
  const double cost_def = __hiloint2double((int)rdl(w, 1), (int)rdl(w, 0));
  const double cost_atk = __hiloint2double((int)rdl(w, 3), (int)rdl(w, 2));
  const int steps = (int)rdl(w, 6), atk_cd = (int)rdl(w, 8), def_cd = (int)rdl(w, 9);
  const int n_en = (int)rdl(w, 10), num_roads = (int)rdl(w, 12);
  int n_tw = (int)rdl(w, 11);
  const bool live = mask_board_live(num_roads);
  const uint64_t ub = (uint64_t)(uint32_t)b;

  if (a.atk_act || a.atk_count) {  // the 12 (road, t < 4) pairs in ascending road * 4 + t: one ballot
    bool ok = false;
    if (lane < 12) ok = mask_summon_ok(lane >> 2, lane & 3, mask_enemy_lv(steps, C), num_roads, atk_cd, n_en, cost_atk, C);
    uint32_t m = (uint32_t)ballot(ok) & 0xfffu;
    const int n_atk = __popc(m);
    int pick = -1;
    if (!sample_idles(sample_u(a.key, ub, SAMPLE_ATK_IDLE), a.atk_idle, n_atk)) {
      for (int k = sample_pick(sample_u(a.key, ub, SAMPLE_ATK_PICK), n_atk); k > 0; --k) m &= m - 1u;
      pick = __builtin_ctz(m);
    }
    // [3][8]: all 4 (none), the chosen road's first slot its type
    if (a.atk_act && lane < 24)
      a.atk_act[(size_t)b * 24 + lane] = pick >= 0 && lane == (pick >> 2) * 8 ? (int64_t)(pick & 3) : (int64_t)4;
    if (a.atk_count && lane == 0) a.atk_count[b] = n_atk;
  }
  if (!a.def_act && !a.def_count) return;

  int n_def = 0, act = -1;  // act: the chosen candidate's index, or nothing
  if (live && mask_cd_open(def_cd)) {  // (wave-uniform)
    const int NP = (6 * NC + 15) >> 4;  // 16-B pieces of the row
    u32x4* const R4 = reinterpret_cast<u32x4*>(R);
    if (lane == 0) {  // the bytes behind the last code: padding, never legal
      const u32x4 pad = {kMaskPad * 0x01010101u, kMaskPad * 0x01010101u, kMaskPad * 0x01010101u, kMaskPad * 0x01010101u};
      R4[NP - 1] = pad;
    }
    wsync();
    // build (ops 0-3) per cell; level-up / destruct (ops 4-5): no tower there
    if (n_tw > TCAP) n_tw = TCAP;  // (never by the step's own stores: an imported header)
    double price[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) price[t] = C.t_price[t][0];
    const uint32_t* const cw = a.cells + (size_t)b * NC;
    auto put_cell = [&](int c, uint32_t word) {
#pragma unroll
      for (int t = 0; t < 4; ++t) R[t * NC + c] = (uint8_t)mask_build_code(cost_def, price[t], word, n_tw);
      R[4 * NC + c] = (uint8_t)mask_lvup_code(false, 0u, cost_def, C);
      R[5 * NC + c] = (uint8_t)mask_destruct_code(false);
    };
    if ((NC & 3) == 0) {  // 16-B loads of four cells (the board's words start 16-B aligned)
      const u32x4* const cw4 = reinterpret_cast<const u32x4*>(cw);
      for (int i = lane; i < NC / 4; i += 64) {
        const u32x4 v = cw4[i];
        put_cell(4 * i + 0, v.x); put_cell(4 * i + 1, v.y); put_cell(4 * i + 2, v.z); put_cell(4 * i + 3, v.w);
      }
    } else {
      for (int c = lane; c < NC; c += 64) put_cell(c, cw[c]);
    }
    wsync();
    if (lane < n_tw) {  // (one tower per cell: no two lanes write the same byte)
      const uint32_t ti = a.tw_inf[(size_t)b * TCAP + lane];
      const int c = tw_cell(ti);
      if (c < NC) {
        R[4 * NC + c] = (uint8_t)mask_lvup_code(true, ti, cost_def, C);
        R[5 * NC + c] = (uint8_t)mask_destruct_code(true);
      }
    }
    wsync();

    // count: this lane's pieces [p0, p0 + P)
    const int P = LT ? SampleRow<LT>::PER_LANE : (NP + 63) >> 6;
    const int p0 = lane * P;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < SampleRow<LT>::PER_LANE; ++j)
      if (j < P && p0 + j < NP) cnt += __popc(legal16(R4[p0 + j]));
    int inc = cnt;  // inclusive prefix sum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(inc, d, 64);
      if (lane >= d) inc += v;
    }
    n_def = (int)rdl((uint32_t)inc, 63);
    if (!sample_idles(sample_u(a.key, ub, SAMPLE_DEF_IDLE), a.def_idle, n_def)) {
      const int k = sample_pick(sample_u(a.key, ub, SAMPLE_DEF_PICK), n_def);
      const bool mine = cnt > 0 && k >= inc - cnt && k < inc;  // exactly one lane
      int found = 0;
      if (mine) {
        int r = k - (inc - cnt);  // the r-th legal byte of this lane's pieces
        bool got = false;
        for (int j = 0; j < P && !got; ++j) {  // (p0 + j < NP: the pieces up to the r-th candidate exist)
          const u32x4 x = R4[p0 + j];
          const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // word by word, so that the candidates come in ascending order
            uint32_t m = mask_legal4(xs[q], true);  // byte i: bit 8 i
            const int c = __popc(m);
            if (got) continue;
            if (r >= c) {
              r -= c;
              continue;
            }
            for (; r > 0; --r) m &= m - 1u;
            found = 16 * (p0 + j) + 4 * q + (__builtin_ctz(m) >> 3);
            got = true;
          }
        }
      }
      const uint64_t own = ballot(mine);
      if (own) act = (int)rdl((uint32_t)found, ctz64(own));
    }
  }

  if (a.def_count && lane == 0) a.def_count[b] = n_def;
  if (!a.def_act) return;
  if (!a.multi) {
    if (lane == 0) a.def_act[b] = act >= 0 ? (int64_t)act : (int64_t)(6 * NC);  // 6 L^2: the no-op
    return;
  }
  // multi-action: the whole [6][L][L] row, zeros and the one chosen flag, in 16-B stores (the
  // row's first and last element alone where the pointer is a multiple of 8 only)
  const int n = 6 * NC;
  int64_t* const row = a.def_act + (size_t)b * n;
  const int h = (reinterpret_cast<uintptr_t>(row) & 8u) ? 1 : 0;
  if (h && lane == 0) row[0] = act == 0 ? 1 : 0;
  const int pairs = (n - h) >> 1;
  for (int i = lane; i < pairs; i += 64) {
    const int e = h + 2 * i;
    const u32x4 v = {e == act ? 1u : 0u, 0u, e + 1 == act ? 1u : 0u, 0u};
    *reinterpret_cast<u32x4*>(row + e) = v;
  }
  if (((n - h) & 1) && lane == 0) row[n - 1] = act == n - 1 ? 1 : 0;
}

}  // namespace

// ids, cap, count, verdict: td_mask_list_kernel's (td_mask_list.hip); ids == nullptr: entry i is
// board i and cap = B.
template <int LT>
__global__ __launch_bounds__(64 * kSampleWaves) void td_sample_kernel(SampleArgs a, const int32_t* ids, int cap,
                                                                      const int32_t* count,
                                                                      const td_list_status* verdict) {
  constexpr int RB = SampleRow<LT>::BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t R[kSampleWaves][RB];
  static_assert(RB % 16 == 0, "every wave's row is 16-B aligned");
  typedef __attribute__((address_space(4))) const int32_t cword_t;
  int n = cap;
  if (verdict) {
    const int code = reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(verdict))[0];
    static_assert(offsetof(td_list_status, code) == 0, "the verdict's first word");
    if (count) n = reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(count))[0];
    n = code ? 0 : n;
  }
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int groups = (n + kSampleWaves - 1) / kSampleWaves, g = (int)blockIdx.x;
  if (g >= groups) return;
  const int i = (a.xcd_map ? xcd_board(g, groups) : g) * kSampleWaves + wave;
  if (i >= n) return;
  const int b = ids ? reinterpret_cast<cword_t*>(reinterpret_cast<uintptr_t>(ids))[i] : i;
  sample_board<LT>(a, b, lane, R[wave]);
}

hipError_t launch_sample(const SampleArgs& a, const int32_t* ids, int cap, const int32_t* count,
                         const td_list_status* verdict, hipStream_t s) {
  const dim3 grid((cap + kSampleWaves - 1) / kSampleWaves), block(64 * kSampleWaves);
  switch (a.L) {
    case 10: hipLaunchKernelGGL(td_sample_kernel<10>, grid, block, 0, s, a, ids, cap, count, verdict); break;
    case 20: hipLaunchKernelGGL(td_sample_kernel<20>, grid, block, 0, s, a, ids, cap, count, verdict); break;
    case 30: hipLaunchKernelGGL(td_sample_kernel<30>, grid, block, 0, s, a, ids, cap, count, verdict); break;
    default: hipLaunchKernelGGL(td_sample_kernel<0>, grid, block, 0, s, a, ids, cap, count, verdict); break;
  }
  return hipGetLastError();
}

}  // namespace td
