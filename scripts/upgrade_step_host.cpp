// upgrade_step_host.cpp -- the integer form of `progress >= enemy_upgrade_at`
// (gym-td_amd/csrc/td_upgrade_step.h) against the division it replaces, as a host program of its
// own: no HIP, no Python, no GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o upgrade_step_host scripts/upgrade_step_host.cpp && ./upgrade_step_host
//
// Without arguments: for every episode limit of {1, 2, 3, 7, 1200, 4095, 4096, 10^6} and every
// threshold of {-1, 0, 0.75, 1, 1 + 2^-52, 2, 1/3, and s / limit exactly and one ulp either side
// for fuzzed s}, `s >= upgrade_step(limit, threshold)` must equal `(double)s / limit >= threshold`
// for every s in [0, limit + 2], at s = 2^31 - 1 and at 1,000 random s.  Prints
// "upgrade_step: N cases ok" and returns 0, or names the first case that went wrong.
//
// With arguments "LIMIT THRESHOLD ..." (the threshold as a C99 hex float): prints upgrade_step
// of each pair, one per line (tests/test_upgrade_step_host.py compares them with Python's own
// division).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../gym-td_amd/csrc/td_upgrade_step.h"

namespace {

long g_cases = 0;
int g_bad = 0;

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {  // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return g_rng * 0x2545f4914f6cdd1dull;
}

void check_one(int32_t limit, double thr, int32_t us, int64_t s) {
  const bool by_division = (double)s / (double)limit >= thr;
  const bool by_count = s >= (int64_t)us;
  ++g_cases;
  if (by_division != by_count && !g_bad++)
    std::printf("FAIL: limit %d threshold %a upgrade_step %d: s = %lld division %d count %d\n", limit, thr, us,
                (long long)s, (int)by_division, (int)by_count);
}

void check_pair(int32_t limit, double thr) {
  const int32_t us = td::upgrade_step(limit, thr);
  for (int64_t s = 0; s <= (int64_t)limit + 2; ++s) check_one(limit, thr, us, s);
  check_one(limit, thr, us, INT32_MAX);
  for (int i = 0; i < 1000; ++i) check_one(limit, thr, us, (int64_t)(next_u64() >> 33));  // [0, 2^31)
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1) {
    for (int i = 1; i + 1 < argc; i += 2)
      std::printf("%d\n", td::upgrade_step((int32_t)std::strtol(argv[i], nullptr, 10), std::strtod(argv[i + 1], nullptr)));
    return 0;
  }
  const int32_t limits[] = {1, 2, 3, 7, 1200, 4095, 4096, 1000000};
  for (int32_t limit : limits) {
    std::vector<double> thr = {-1.0, 0.0, 0.75, 1.0, 1.0 + std::ldexp(1.0, -52), 2.0, 1.0 / 3.0};
    // s / limit exactly and one ulp either side: the ends, the limit's neighbours and fuzzed s
    std::vector<int64_t> at = {0, 1, limit - 1, limit, (int64_t)limit + 1, (int64_t)limit + 2};
    for (int i = 0; i < 6; ++i) at.push_back((int64_t)(next_u64() % ((uint64_t)limit + 3)));
    for (int64_t s : at) {
      if (s < 0) continue;
      const double q = (double)s / (double)limit;
      thr.push_back(q);
      thr.push_back(std::nextafter(q, -INFINITY));
      thr.push_back(std::nextafter(q, INFINITY));
    }
    for (double t : thr) check_pair(limit, t);
  }
  // no step count reaches the threshold: INT32_MAX, and every count below it agrees
  {
    const int32_t us = td::upgrade_step(7, 1e300);
    ++g_cases;
    if (us != INT32_MAX && !g_bad++) std::printf("FAIL: an unreachable threshold gave %d\n", us);
    for (int64_t s : {(int64_t)0, (int64_t)7, (int64_t)INT32_MAX - 1}) check_one(7, 1e300, us, s);
  }
  if (g_bad) return 1;
  std::printf("upgrade_step: %ld cases ok\n", g_cases);
  return 0;
}
