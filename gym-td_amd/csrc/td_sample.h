// td_sample.h -- the rule of td_sample_actions: the random word of a draw and the choice made
// with it; below it the rule of td_sample_weighted on the same words.  Plain C++ that builds with
// and without HIP: shared by the sample kernels (td_sample.hip, td_sample_w.hip), td_capi.hip (the
// call's key) and scripts/sample_rule_host.cpp / sample_weighted_rule_host.cpp, which run it
// alone; gym_TD/sampling.py restates it in numpy.
//
//   sm(z)  : splitmix64's output step on z + 0x9E3779B97F4A7C15 (all mod 2^64)
//   word(seed, ticket, b, j) = sm( sm( sm(seed) + ticket ) + 4 b + j )     b = board id, j = draw
//   u = word >> 32
//   j = 0: the defender idles iff u < def_idle     j = 1: the defender's pick  k = (u * n_def) >> 32
//   j = 2: the attacker idles iff u < atk_idle     j = 3: the attacker's pick  k = (u * n_atk) >> 32
//
// The sampler is stateless: a draw is a function of (seed, ticket, board id, draw) and of
// nothing a handle keeps, so a call is reproducible and two copies of one board at different
// ids draw differently.  The multiply-shift pick maps 2^32 values of u onto n candidates: each
// candidate gets floor(2^32 / n) or one more of them, a bias of at most n / 2^32 (n <= 6,144:
// 1.5e-6) -- no rejection loop.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TD_SAMPLE_HD __host__ __device__
#else
#define TD_SAMPLE_HD
#endif

namespace td {

enum : int { SAMPLE_DEF_IDLE = 0, SAMPLE_DEF_PICK = 1, SAMPLE_ATK_IDLE = 2, SAMPLE_ATK_PICK = 3, SAMPLE_DRAWS = 4 };

TD_SAMPLE_HD inline uint64_t sample_sm(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// What a call's seed and ticket come to, computed once on the host: the kernel's argument.
TD_SAMPLE_HD inline uint64_t sample_key(uint64_t seed, uint64_t ticket) { return sample_sm(sample_sm(seed) + ticket); }

TD_SAMPLE_HD inline uint64_t sample_word_of_key(uint64_t key, uint64_t b, int j) {
  return sample_sm(key + (uint64_t)SAMPLE_DRAWS * b + (uint64_t)j);
}
TD_SAMPLE_HD inline uint64_t sample_word(uint64_t seed, uint64_t ticket, uint64_t b, int j) {
  return sample_word_of_key(sample_key(seed, ticket), b, j);
}
TD_SAMPLE_HD inline uint32_t sample_u(uint64_t key, uint64_t b, int j) { return (uint32_t)(sample_word_of_key(key, b, j) >> 32); }

// A side chooses nothing: no candidate, or the idle draw fires (idle in units of 2^-32).
TD_SAMPLE_HD inline bool sample_idles(uint32_t u, uint32_t idle, int n) { return n <= 0 || u < idle; }
// The index of the pick among n >= 1 candidates in ascending order.
TD_SAMPLE_HD inline int sample_pick(uint32_t u, int n) { return (int)(((uint64_t)u * (uint64_t)(uint32_t)n) >> 32); }

// ---- the rule of td_sample_weighted: integers only, so that a sum has no order.
//
//   q(w) = 0 unless w > 0 (NaN, -0, negatives, 0), else (uint32) trunc(min(w, 1) * 2^31): the f32
//          product by a power of two is exact, +inf and everything above 1 give 2^31, subnormals
//          and everything below 2^-31 give 0
//   m(e) = q(w[e]) where entry e is legal (the side's always-legal entry comes last), else 0
//   S    = sum of m, a uint64 (< 2^44: at most 6,145 entries of at most 2^31)
//   S == 0: the always-legal entry, mass (0, 0)
//   else r = (word * S) >> 64 with the draw's whole 64-bit word (j = 1 the defender, j = 3 the
//          attacker; no idle draw: choosing nothing is the always-legal entry's weight), and the
//          pick is the smallest e whose inclusive prefix sum of m exceeds r; mass (m(e), S)
// r < S, so there is such an e and m(e) > 0.  Each entry gets floor(m 2^64 / S) or one more of the
// 2^64 words: the pick's probability is m / S up to S / 2^64 < 2^-20.
TD_SAMPLE_HD inline uint32_t sample_quant(float w) {
  if (!(w > 0.0f)) return 0u;
  return (uint32_t)((w < 1.0f ? w : 1.0f) * 2147483648.0f);
}
TD_SAMPLE_HD inline uint64_t sample_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}
// The threshold r of a draw's word against the total S >= 1.
TD_SAMPLE_HD inline uint64_t sample_threshold(uint64_t word, uint64_t S) { return sample_mulhi64(word, S); }
// The rule over n entries in order (m[e] already 0 where e is illegal; the always-legal entry is
// m[n - 1]): the pick, and its mass (m, S) or (0, 0) in mass[2] where mass != nullptr.  What a
// kernel does wave-wide, restated for one thread: scripts/sample_weighted_rule_host.cpp runs it.
TD_SAMPLE_HD inline int sample_pick_weighted(const uint32_t* m, int n, uint64_t word, uint64_t* mass) {
  uint64_t S = 0;
  for (int e = 0; e < n; ++e) S += m[e];
  int pick = n - 1;
  uint64_t mp = 0;
  if (S) {
    const uint64_t r = sample_threshold(word, S);
    uint64_t c = 0;
    for (int e = 0; e < n; ++e) {
      c += m[e];
      if (c > r) {
        pick = e;
        mp = m[e];
        break;
      }
    }
  }
  if (mass) {
    mass[0] = mp;
    mass[1] = S;
  }
  return pick;
}

}  // namespace td
