// td_sample.hip -- td_sample_kernel: one uniformly drawn legal action per side and board
// (td_sample_actions, td_sample_actions_boards, td_sample_actions_boards_dev), by td_sample.h's
// rule over td_mask.h's verdicts.
//
// Shape: td_mask_list_kernel's -- one wave per entry, kSampleWaves entries per workgroup under
// the XCD-contiguous group map, each wave with an LDS row of its own that only wsync() orders,
// the list's length and the wave's entry as td_list_dev.h makes them.  ids == nullptr serves
// every board: entry i is board i.
//
// Per board the wave puts the row of fail codes together in LDS with mask_board's row build
// (td_mask_body.h: header words, cell pass, tower lanes) and does not store it.  Lane l owns the P
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
#include "td_mask_body.h"
#include "td_sample.h"

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
  const BoardView& v = a.v;
  const int L = LT ? LT : v.L, NC = L * L;
  const TdDevCfg& C = *v.cfg;

  const HdrWords hd(v.hdr + b, lane);
  const double cost_def = hd.cost_def();
  const double cost_atk = hd.cost_atk();
  const int steps = hd.steps(), atk_cd = hd.atk_cd(), def_cd = hd.def_cd();
  const int n_en = hd.n_en(), num_roads = hd.num_roads();
  int n_tw = hd.n_tw();
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
    if (n_tw > TCAP) n_tw = TCAP;  // (never by the step's own stores: an imported header)
    TD_ROW_CELLS(R)
    wsync();
    TD_ROW_TOWERS(R)
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
  if (!v.multi) {
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
  const int n = list_length(cap, count, verdict);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  int i;
  if (!list_wave_entry<kSampleWaves>(a.v.xcd_map, n, wave, &i)) return;
  const int b = ids ? list_word(ids, i) : i;
  sample_board<LT>(a, b, lane, R[wave]);
}

hipError_t launch_sample(const SampleArgs& a, const int32_t* ids, int cap, const int32_t* count,
                         const td_list_status* verdict, hipStream_t s) {
  const dim3 grid((cap + kSampleWaves - 1) / kSampleWaves), block(64 * kSampleWaves);
  with_side(a.v.L, [&](auto lt) {
    hipLaunchKernelGGL(td_sample_kernel<decltype(lt)::value>, grid, block, 0, s, a, ids, cap, count, verdict);
  });
  return hipGetLastError();
}

}  // namespace td
