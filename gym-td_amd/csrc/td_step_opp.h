// td_step_opp.h -- the built-in opponents and their random streams.
// What belongs here: the wave-parallel CPython MT19937 (WaveMt), the choice between the
// board's CPython and numpy streams (OppRng, with_opp_rng), and the reference's scripted
// opponents random_enemy_lv* / random_tower_lv* (TDGymBasic.py:81-292), which act through
// the tower operations and summon_cluster of td_step_rules.h.
#pragma once
#include "td_kernels.h"
#include "td_rng.h"
#include "td_step_rules.h"
#include "td_step_state.h"
#include "td_wave.h"

namespace td {

// ---------------------------------------------------------------------------
// CPython MT19937 for the built-in opponent, state in HBM, wave-parallel twist
// ---------------------------------------------------------------------------
// CPython MT19937 with a lazy twist: word p of a new block is twisted when it is
// drawn.  In sequential order word p of the new block depends on old[p], old[p+1]
// (new[0] for p = 623) and old[p+397] (p < 227) or new[p-227] (p >= 227), all of
// which are available when p is drawn in order, so draws are bit-identical to
// CPython's block twist without ever running the 624-word loop in the step.
// State: w[0..623], pos = w[624], tw = w[625] (words [tw, 624) not yet twisted).
struct WaveMt {
  uint32_t* w;
  uint32_t pos, tw;
  uint32_t cache = 0, cbase = 0, cn = 0;  // lane j: tempered output for position cbase + j (j < cn)
  __device__ __forceinline__ void wrap() {
    tw = 0;
    pos = 0;
  }

  // Pre-draws still unused at the current position (0 after a block wrap).
  __device__ __forceinline__ uint32_t cached_left() const {
    const uint32_t d = pos - cbase;
    return d < cn ? cn - d : 0u;
  }
  // Pre-draw the next up-to-HOT_CACHE words in parallel, one per lane, for the next
  // step: issue() starts the loads, finish() (at the end of the step) lazily
  // twists, stores and tempers them -- the memory latency overlaps the step.
  uint32_t pa = 0, pnb = 0, pfar = 0;
  bool plazy = false, pmine = false;
  __device__ __forceinline__ void prefetch_issue(int lane) {
    if (pos >= (uint32_t)MT_N) wrap();
    cbase = pos;
    cn = (uint32_t)MT_N - pos < (uint32_t)HOT_CACHE ? (uint32_t)MT_N - pos : (uint32_t)HOT_CACHE;
    const uint32_t q = pos + (uint32_t)lane;
    pmine = (uint32_t)lane < cn;
    plazy = pmine && q >= tw;
    if (pmine) {
      pa = w[q];
      if (plazy) {
        // word q (< pos + 8 <= tw + 8) needs new[q - 227], twisted in an earlier step
        pnb = w[q == MT_N - 1 ? 0u : q + 1u];
        pfar = w[q < (uint32_t)(MT_N - MT_M) ? q + MT_M : q - (MT_N - MT_M)];
      }
    }
  }
  __device__ __forceinline__ void prefetch_finish(int lane) {
    const uint32_t q = cbase + (uint32_t)lane;
    uint32_t y = pa;
    if (plazy) {
      const uint32_t yy = (pa & 0x80000000u) | (pnb & 0x7fffffffu);
      y = pfar ^ (yy >> 1) ^ ((yy & 1u) ? 0x9908b0dfu : 0u);
      w[q] = y;  // after every lane's loads (data dependency)
    }
    if (cbase + cn > tw) tw = cbase + cn;
    cache = pmine ? mt_temper(y) : 0u;
  }
  __device__ __forceinline__ void prefetch(int lane) {
    prefetch_issue(lane);
    prefetch_finish(lane);
  }

  // Early pre-draw (the small kernels): the loads of the window [p0, p0 + 16)
  // at the position p0 the step starts from are issued right after the hot record is in,
  // before any of the step's stores -- their wait at the step's end then neither waits on
  // the memory latency nor, through the in-order vmcnt, on the step's own stores.  The step
  // draws d <= 8 words in practice; the next pre-drawn outputs are the window's lanes
  // d .. d + 7.  A lazily twisted word the step's slow path twisted meanwhile is twisted
  // again from the same old words (same value); a window the step outran (d > 8, or a
  // block wrap) falls back to the late pre-draw.
  static constexpr uint32_t kEarlyWin = 16;
  uint32_t ep0 = ~0u;  // the window's first position (~0u: none)
  __device__ __forceinline__ void early_issue(int lane) {
    // (pos <= tw always: the window's lazy words need old or already twisted words only)
    if (pos + kEarlyWin > (uint32_t)MT_N) return;
    ep0 = pos;
    const uint32_t q = pos + (uint32_t)lane;
    pmine = (uint32_t)lane < kEarlyWin;
    plazy = pmine && q >= tw;
    if (pmine) {
      pa = w[q];
      if (plazy) {
        pnb = w[q == MT_N - 1 ? 0u : q + 1u];
        pfar = w[q < (uint32_t)(MT_N - MT_M) ? q + MT_M : q - (MT_N - MT_M)];
      }
    }
  }
  __device__ __forceinline__ bool early_ok() const { return ep0 != ~0u && pos - ep0 <= kEarlyWin - 8u; }
  // The early window's outputs, or (outran: d > 8, a block wrap, no window) a late
  // pre-draw -- one tail for both, so that no field is stored on one branch only (LLVM
  // merges such stores through a pointer phi, and the object no longer fits registers).
  __device__ __forceinline__ void early_finish(int lane) {
    uint32_t base, n, d;
    if (early_ok()) {
      base = ep0; n = kEarlyWin; d = pos - ep0;
    } else {
      prefetch_issue(lane);  // (wraps if due; cbase = pos)
      base = cbase; n = cn; d = 0u;
    }
    const uint32_t q = base + (uint32_t)lane;
    uint32_t y = pa;
    if (plazy) {
      const uint32_t yy = (pa & 0x80000000u) | (pnb & 0x7fffffffu);
      y = pfar ^ (yy >> 1) ^ ((yy & 1u) ? 0x9908b0dfu : 0u);
      w[q] = y;  // (a word the step's slow path twisted meanwhile: the same value again)
    }
    if (base + n > tw) tw = base + n;
    const uint32_t t = pmine ? mt_temper(y) : 0u;
    cache = (uint32_t)__shfl((int)t, (int)(((uint32_t)lane + d) & 63u));
    cbase = pos;
    cn = n - d < (uint32_t)HOT_CACHE ? n - d : (uint32_t)HOT_CACHE;
  }

  __device__ __forceinline__ uint32_t next() {
    const uint32_t d = pos - cbase;
    if (d < cn) {
      ++pos;
      return rdl(cache, (int)d);  // d is wave-uniform: a scalar read, no LDS round trip
    }
    if (pos >= (uint32_t)MT_N) { wrap(); cn = 0; }
    uint32_t y;
    if (pos >= tw) {
      const uint32_t a = w[pos];
      const uint32_t nb = w[pos == MT_N - 1 ? 0u : pos + 1u];
      const uint32_t far = w[pos < (uint32_t)(MT_N - MT_M) ? pos + MT_M : pos - (MT_N - MT_M)];
      const uint32_t yy = (a & 0x80000000u) | (nb & 0x7fffffffu);
      y = far ^ (yy >> 1) ^ ((yy & 1u) ? 0x9908b0dfu : 0u);
      w[pos] = y;  // every lane stores the same word
      tw = pos + 1;
    } else {
      y = w[pos];
    }
    ++pos;
    return mt_temper(y);
  }
  __device__ __forceinline__ int64_t randbelow(int64_t n) {
    if (n <= 0) return 0;  // never reached on a valid board (guards against an unbounded loop)
    int k = 64 - __builtin_clzll((unsigned long long)n);
    uint32_t r = next() >> (32 - k);
    while ((int64_t)r >= n) r = next() >> (32 - k);
    return r;
  }
  __device__ __forceinline__ int64_t randint(int64_t a, int64_t b) { return a + randbelow(b - a + 1); }
  // numpy legacy RandomState.randint(lo, hi) (hi exclusive): masked rejection on 32-bit
  // outputs, no draw when hi - lo == 1; also shuffle's random_interval(i) = np_randint(0, i + 1)
  __device__ __forceinline__ int64_t np_randint(int64_t lo, int64_t hi) {
    if (hi <= lo + 1) return lo;
    const uint32_t rng = (uint32_t)(hi - lo - 1);
    uint32_t mask = rng;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    uint32_t v = next() & mask;
    while (v > rng) v = next() & mask;
    return lo + (int64_t)v;
  }
  __device__ __forceinline__ double random() {
    uint32_t x = next() >> 5, y = next() >> 6;
    return (x * 67108864.0 + y) * (1.0 / 9007199254740992.0);
  }
};

// The built-in opponents' random source (TDGymBasic.py:81-292).  random_agent=True
// (NP = false): the board's CPython stream.  random_agent=False (NP = true): the
// board's numpy layout stream (the one reset() draws roads from), except the destruct
// branch's tower index, which the reference still draws from CPython random (:191,
// :287).  Each method is one call site shape of the reference: ri(lo, hi) =
// random.randint(lo, hi) | np_random.randint(lo, hi + 1).  NP is a template argument,
// not a nullable pointer: a pointer chosen between two locals at run time would keep
// both streams in scratch memory.
template <bool NP>
struct OppRng {
  WaveMt& py;
  WaveMt& np;  // == py when !NP
  __device__ __forceinline__ int64_t ri(int64_t lo, int64_t hi) {
    if constexpr (NP) return np.np_randint(lo, hi + 1); else return py.randint(lo, hi);
  }
  __device__ __forceinline__ double rnd() {
    if constexpr (NP) return np.random(); else return py.random();
  }
  // random.shuffle's randbelow(i + 1) | np shuffle's random_interval(i)
  __device__ __forceinline__ int64_t shuffle_j(int64_t i) {
    if constexpr (NP) return np.np_randint(0, i + 1); else return py.randbelow(i + 1);
  }
  // random_enemy_lv0's cluster slot: random.randint(0, types) (:85) | np_random.randint(0, types) (:88)
  __device__ __forceinline__ int64_t slot(int64_t types) {
    if constexpr (NP) return np.np_randint(0, types); else return py.randint(0, types);
  }
};

// Runs f(OppRng<...>&) on the stream random_agent selects.  random_agent=False: board
// b's numpy layout stream, loaded from and stored back to its MT record (np_mt).
template <class F>
__device__ __forceinline__ void with_opp_rng(const StepArgs& a, int b, int lane, WaveMt& R, F&& f) {
  if (a.opp_np) {
    uint32_t* const npw = a.np_mt + (size_t)b * OPP_WORDS;
    WaveMt N{npw, npw[MT_N], npw[MT_N + 1]};
    N.cbase = N.pos;
    OppRng<true> G{R, N};
    f(G);
    if (lane == 0) { npw[MT_N] = N.pos; npw[MT_N + 1] = N.tw; }
  } else {
    OppRng<false> G{R, R};
    f(G);
  }
}

// ---------------------------------------------------------------------------
// built-in opponents
// ---------------------------------------------------------------------------
template <int NC, class Rng>
__device__ __forceinline__ void opponent_enemy(Smem<NC>& S, U& u, const Ctx& x, Rng& R, int difficulty) {
  // random_enemy_lv0 / lv1 (TDGymBasic.py:81-108)
  if (u.atk_cd != 0) return;
  uint32_t types = 0;
  int road;
  if (difficulty == 0) {
    for (int k = 0; k < 8; ++k) types |= (uint32_t)R.slot(4) << (4 * k);
    road = (int)R.ri(0, u.num_roads - 1);
  } else {
    const uint32_t t = (uint32_t)R.ri(0, 3);
    road = (int)R.ri(0, u.num_roads - 1);
    types = t * 0x11111111u;
  }
  summon_cluster(S, u, x, types, road, nullptr);
  wsync();
  u.atk_cd = x.C.atk_interval;  // the (ok, real) tuple is always truthy
}

template <int NC, class Rng>
__device__ __forceinline__ void opponent_tower_lv0(Smem<NC>& S, U& u, const Ctx& x, Rng& R) {
  // random_tower_lv0 (TDGymBasic.py:111-122)
  if (u.def_cd != 0) return;
  int r = (int)R.ri(0, x.L - 1);
  int c = (int)R.ri(0, x.L - 1);
  int t = (int)R.ri(0, 3);
  if (tower_build(S, u, x, t, r * x.L + c) == FC_OK) u.def_cd = x.C.def_interval;
}

// random_tower_lv1 / lv2 (TDGymBasic.py:124-292).
template <int NC, class Rng>
__device__ __forceinline__ void build_near_road(Smem<NC>& S, U& u, const Ctx& x, Rng& R, int t, bool draw_type) {
  // road cells in row-major order, then random.shuffle (Fisher-Yates on randbelow)
  // The list lives in the sort-key scratch as cell indices (<= L*L <= 4096 > 4*ECAP,
  // so it is kept in the group map instead: grp has 4*NC bytes -> store u16 cells).
  uint16_t* cells = reinterpret_cast<uint16_t*>(&S.grp[0][0]);
  int nroad = 0;
  for (int base = 0; base < x.NCr; base += 64) {
    int c = base + x.lane;
    bool isr = c < x.NCr && (S.cell[c] & 1u);
    uint64_t m = ballot(isr);
    const uint64_t lt = (x.lane == 0) ? 0ull : (~0ull >> (64 - x.lane));
    if (isr) cells[nroad + popc64(m & lt)] = (uint16_t)c;
    nroad += popc64(m);
  }
  wsync();
  for (int i = nroad - 1; i >= 1; --i) {
    int j = (int)R.shuffle_j(i);
    if (x.lane == 0) { uint16_t tmp = cells[i]; cells[i] = cells[j]; cells[j] = tmp; }
    wsync();
  }
  if (draw_type) t = (int)R.ri(0, 3);
  for (int i = 0; i < nroad; ++i) {
    int k = (int)R.ri(0, 24);
    int dr = k / 5 - 2, dc = k % 5 - 2;
    int cc = cells[i];
    const int rc = div_side(cc, x.Lm);
    int r = rc + dr, c = cc - rc * x.L + dc;
    if (r < 0 || r >= x.L || c < 0 || c >= x.L) continue;
    int fc = tower_build(S, u, x, t, r * x.L + c);
    if (fc == FC_OK) { u.def_cd = x.C.def_interval; return; }
    if (fc == FC_COST) return;
  }
}

template <int NC, class Rng>
__device__ __forceinline__ void upgrade_or_destruct(Smem<NC>& S, U& u, const Ctx& x, Rng& R, int act) {
  if (u.nt == 0) return;
  if (act == 1) {
    int id = (int)R.ri(0, u.nt - 1);
    int cell = (int)(S.tInf[id] & 0xfffu);
    if (tower_lvup(S, u, x, cell) == FC_OK) u.def_cd = x.C.def_interval;
  } else {
    if (R.rnd() > 0.01) return;
    int id = (int)R.py.randint(0, u.nt - 1);  // CPython random whatever random_agent is (:187, :191)
    int cell = (int)(S.tInf[id] & 0xfffu);
    if (tower_destruct(S, u, x, cell) == FC_OK) u.def_cd = x.C.def_interval;
  }
}

template <int NC, class Rng>
__device__ __forceinline__ void opponent_tower(Smem<NC>& S, U& u, const Ctx& x, Rng& R, int difficulty) {
  if (difficulty == 0) { opponent_tower_lv0(S, u, x, R); return; }
  if (u.def_cd != 0) return;
  int act = (int)R.ri(0, 2);
  if (act != 0) { upgrade_or_destruct(S, u, x, R, act); return; }
  if (difficulty == 1) { build_near_road(S, u, x, R, 0, true); return; }
  // lv2: tower type from the enemy type mix (TDGymBasic.py:217-240)
  if (u.n == 0) return;
  int cnt[4] = {0, 0, 0, 0};
  for (int i = 0; i < u.n; ++i) cnt[en_type(S.eInf[i])] += 1;
  // np.unique -> present types ascending; ratio = nums.astype(float32) / np.sum(nums):
  // float32 array / int64 scalar promotes to float64 (NEP 50), so the ratio is an f64 quotient
  int types[4], nt = 0;
  for (int t = 0; t < 4; ++t) if (cnt[t]) types[nt++] = t;
  double p = R.rnd();
  int chosen = -1;
  for (int i = 0; i < 4; ++i) {
    if (i >= nt) { u.flags |= FLAG_BAD_ACTION; break; }  // the reference raises IndexError here
    double ratio = ddiv((double)cnt[types[i]], (double)u.n);
    if (p < ratio) { chosen = types[i]; break; }
    p = dsub(p, ratio);
  }
  if (chosen < 0) return;
  const int remap[4] = {2, 0, 1, 0};
  int t = remap[chosen];
  if (R.rnd() < 0.2) t = 3;
  build_near_road(S, u, x, R, t, false);
}

}  // namespace td
