// td_sample_w.hip -- td_sample_weighted_kernel: one legal action per side and board drawn in
// proportion to the caller's weights (td_sample_weighted, td_sample_weighted_boards,
// td_sample_weighted_boards_dev), by td_sample.h's integer rule over td_mask.h's verdicts.
//
// Shape: td_sample_kernel's -- one wave per entry, kSampleWaves entries per workgroup under the
// XCD-contiguous group map, each wave with an LDS row of its own that only wsync() orders, the
// list's length and the wave's entry as td_list_dev.h makes them; ids == nullptr serves every
// board.  The row of fail codes is mask_board's row build (td_mask_body.h), not stored; while the
// defender's cool-down is closed, and on a board that was never reset, it is not built and the
// weight row is not read (but its last float, where the mass is wanted).
//
// The weight row is the call's traffic.  The entries 0 .. 6 L^2 (the no-op last) are taken in
// rounds of 256: in round k lane l owns the four entries of word 64 k + l -- one ds_read_b32 of
// the codes, and of the weights one 16-B load per lane (1 KiB per wave and instruction) where
// the row starts on a multiple of 16, else up to four 4-B loads at the same addresses; only
// words with a legal byte are loaded, and nothing behind entry 6 L^2.  The quantised weights of
// a round are summed in uint64 over the wave and the total kept by lane k; a wave scan over
// those totals gives S, the draw's threshold r and the round that holds the pick; that round's
// weights are loaded again (from cache), a second scan gives the lane, which walks its four
// entries.  Integer sums: the shape of the reduction does not show in the result.
// The attacker's 13 entries are 13 lanes and one scan.
//
// Budget: no scratch; LDS = kSampleWaves * SampleWRow<L>::BYTES, the uniform sampler's row (the
// no-op has no byte in it: its verdict is a constant): 2,432 / 9,600 / 21,632 / 24,576 B at
// L = 10 / 20 / 30 / generic.
#include "td_mask_body.h"
#include "td_sample.h"

namespace td {

namespace {

template <int LT>
struct SampleWRow {
  static constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  static constexpr int BYTES = (6 * NC + 15) & ~15;
  static constexpr int ROUNDS = ((6 * NC + 1 + 3) / 4 + 63) / 64;  // of 64 words of four entries
};
static_assert(SampleWRow<0>::ROUNDS <= 64, "a round's total lives in the lane of its number");

__device__ __forceinline__ uint64_t rdl64(uint64_t v, int l) {
  return ((uint64_t)rdl((uint32_t)(v >> 32), l) << 32) | (uint64_t)rdl((uint32_t)v, l);
}
// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint64_t scan64(uint64_t x, int lane) {
  uint64_t inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t v = (uint64_t)__shfl_up((unsigned long long)inc, (unsigned)d, 64);
    if (lane >= d) inc += v;
  }
  return inc;
}

// What a lane holds of a round: the legal bytes of its word (byte q: bit 8 q) and their weights.
struct RoundW {
  uint32_t legal;
  float f[4];
  __device__ __forceinline__ uint32_t m(int q) const { return (legal >> (8 * q)) & 1u ? sample_quant(f[q]) : 0u; }
  __device__ __forceinline__ uint64_t sum() const { return (uint64_t)m(0) + m(1) + m(2) + m(3); }
};

// R: the wave's own SampleWRow<LT>::BYTES of LDS, 16-B aligned; only wsync() orders its accesses.
template <int LT>
__device__ __forceinline__ void sample_weighted_board(const SampleWArgs& a, int b, int lane, uint8_t* const R) {
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

  if (a.atk_act) {  // entry e < 12: the pair (e >> 2, e & 3); entry 12: nothing, always legal
    bool ok = lane == 12;
    if (lane < 12) ok = mask_summon_ok(lane >> 2, lane & 3, mask_enemy_lv(steps, C), num_roads, atk_cd, n_en, cost_atk, C);
    uint32_t m = 0;
    if (ok) m = sample_quant(a.atk_w[(size_t)b * 13 + lane]);
    const uint64_t inc = scan64(m, lane);
    const uint64_t S = rdl64(inc, 63);
    int pick = 12;
    uint32_t mp = 0;
    if (S) {
      const uint64_t r = sample_threshold(sample_word_of_key(a.key, ub, SAMPLE_ATK_PICK), S);
      const int own = ctz64(ballot(inc > r));  // (r < S: there is one, and its m > 0)
      pick = own;
      mp = rdl(m, own);
    }
    // [3][8]: all 4 (none), the chosen road's first slot its type
    if (lane < 24) a.atk_act[(size_t)b * 24 + lane] = pick < 12 && lane == (pick >> 2) * 8 ? (int64_t)(pick & 3) : (int64_t)4;
    if (a.atk_mass && lane < 2) a.atk_mass[(size_t)b * 2 + lane] = lane ? S : (uint64_t)mp;
  }
  if (!a.def_act) return;

  const int NE = 6 * NC + 1;  // entries: the no-op is the last
  const float* const w = a.def_w + (size_t)b * a.def_pitch;
  int act = NE - 1;
  uint32_t mp = 0;
  uint64_t S = 0;
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

    const int NW = (NE + 3) >> 2;  // words of four entries
    const int K = LT ? SampleWRow<LT>::ROUNDS : (NW + 63) >> 6;
    const uint32_t* const R32 = reinterpret_cast<const uint32_t*>(R);
    const bool al16 = (reinterpret_cast<uintptr_t>(w) & 15u) == 0;  // (wave-uniform)
    auto load_round = [&](int k) {
      RoundW x = {0u, {0.0f, 0.0f, 0.0f, 0.0f}};
      const int i = 64 * k + lane;
      if (i >= NW) return x;
      const uint32_t codes = i < 4 * NP ? R32[i] : kMaskPad * 0x01010101u;
      x.legal = mask_legal4(codes, true);
      if (i == (NE - 1) >> 2) x.legal |= 1u << (8 * ((NE - 1) & 3));  // the no-op
      if (!x.legal) return x;
      const int e = 4 * i;  // (a legal byte is an entry < NE: nothing behind the row's NE floats is read)
      if (al16 && e + 4 <= NE) {
        const float4 f = *reinterpret_cast<const float4*>(w + e);
        x.f[0] = f.x; x.f[1] = f.y; x.f[2] = f.z; x.f[3] = f.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((x.legal >> (8 * q)) & 1u) x.f[q] = w[e + q];
      }
      return x;
    };

    uint64_t T = 0;  // lane k: round k's total
    RoundW cur = load_round(0);
    for (int k = 0; k < K; ++k) {
      const RoundW nxt = load_round(k + 1);  // (round K: no word)
      const uint64_t tot = rdl64(scan64(cur.sum(), lane), 63);
      if (lane == k) T = tot;
      cur = nxt;
    }
    const uint64_t incT = scan64(T, lane);
    S = rdl64(incT, 63);
    if (S) {
      const uint64_t r = sample_threshold(sample_word_of_key(a.key, ub, SAMPLE_DEF_PICK), S);
      const int ks = ctz64(ballot(incT > r));  // the round that holds the pick (r < S: there is one)
      const uint64_t base = rdl64(incT - T, ks);
      const RoundW x = load_round(ks);  // again, from cache
      const uint64_t s = x.sum();
      const uint64_t inc = base + scan64(s, lane);
      const int own = ctz64(ballot(inc > r));
      uint32_t found = 0, mf = 0;
      if (lane == own) {
        uint64_t c = inc - s;
        bool got = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          c += x.m(q);
          if (!got && c > r) {
            found = (uint32_t)(4 * (64 * ks + lane) + q);
            mf = x.m(q);
            got = true;
          }
        }
      }
      act = (int)rdl(found, own);
      mp = rdl(mf, own);
    }
  } else if (a.def_mass) {  // only the no-op can carry mass
    const uint32_t m = sample_quant(w[NE - 1]);
    S = m;
    mp = m;
  }

  if (lane == 0) a.def_act[b] = (int64_t)act;
  if (a.def_mass && lane < 2) a.def_mass[(size_t)b * 2 + lane] = lane ? S : (uint64_t)mp;
}

}  // namespace

// ids, cap, count, verdict: td_sample_kernel's (td_sample.hip); ids == nullptr: entry i is board i
// and cap = B.
template <int LT>
__global__ __launch_bounds__(64 * kSampleWaves) void td_sample_weighted_kernel(SampleWArgs a, const int32_t* ids, int cap,
                                                                               const int32_t* count,
                                                                               const td_list_status* verdict) {
  constexpr int RB = SampleWRow<LT>::BYTES;
  __shared__ __attribute__((aligned(16))) uint8_t R[kSampleWaves][RB];
  static_assert(RB % 16 == 0, "every wave's row is 16-B aligned");
  const int n = list_length(cap, count, verdict);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  int i;
  if (!list_wave_entry<kSampleWaves>(a.v.xcd_map, n, wave, &i)) return;
  const int b = ids ? list_word(ids, i) : i;
  sample_weighted_board<LT>(a, b, lane, R[wave]);
}

hipError_t launch_sample_weighted(const SampleWArgs& a, const int32_t* ids, int cap, const int32_t* count,
                                  const td_list_status* verdict, hipStream_t s) {
  const dim3 grid((cap + kSampleWaves - 1) / kSampleWaves), block(64 * kSampleWaves);
  with_side(a.v.L, [&](auto lt) {
    hipLaunchKernelGGL(td_sample_weighted_kernel<decltype(lt)::value>, grid, block, 0, s, a, ids, cap, count, verdict);
  });
  return hipGetLastError();
}

}  // namespace td
