// td_sample.h -- the rule of td_sample_actions: the random word of a draw and the choice made
// with it.  Plain C++ that builds with and without HIP: shared by the sample kernel
// (td_sample.hip), td_capi.hip (the call's key) and scripts/sample_rule_host.cpp, which runs it
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

}  // namespace td
