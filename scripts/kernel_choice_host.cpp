// kernel_choice_host.cpp -- the TD_KERNEL_AUTO rule and the write-through rule
// (gym-td_amd/csrc/td_kernel_choice.h) at every boundary of their table, as a host program of its
// own: no HIP, no Python, no GPU.  The rules decide which kernel the bench runs on; a boundary one
// board off would pass every parity test and show only as a slower step.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o kernel_choice_host scripts/kernel_choice_host.cpp && ./kernel_choice_host
//
// Kinds: 0 large, 1 small, 2 small2.  The resident counts are inputs of the rule: 8,192 boards with
// one wave each and 4,096 with two at L = 10 (256 CUs x 4 SIMDs x 8 waves), half of them at L = 20 / 30.
// Prints "kernel_choice: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <initializer_list>

#define __host__
#define __device__
#include "../gym-td_amd/csrc/td_kernel_choice.h"

namespace {

int g_cases = 0, g_bad = 0;
const char* kModes[3] = {"TD-def", "TD-atk", "TD-2p"};

void expect_kind(int fmt, int L, int mode, int multi, int r1, int r2, int B, int want) {
  const int got = td::auto_kernel_kind(L, mode, multi, fmt, B, r1, r2);
  ++g_cases;
  if (got != want) {
    if (!g_bad++)
      std::printf("FAIL kind: %s L %d %s %s residents %d / %d B %d: got %d want %d\n", fmt ? "float16" : "float32", L,
                  kModes[mode], multi ? "multi-action" : "single action", r1, r2, B, got, want);
  }
}

void expect_wt(int fmt, int L, int kind, int B, int want) {
  const int got = td::obs_write_through(kind, L, fmt, B);
  ++g_cases;
  if (got != want) {
    if (!g_bad++)
      std::printf("FAIL write-through: %s L %d kind %d B %d: got %d want %d\n", fmt ? "float16" : "float32", L, kind, B,
                  got, want);
  }
}

// the float32 rule's rows at L = 20 / 30, which float16 shares
void rows_L20_L30(int fmt) {
  const int r1 = 4096, r2 = 2048;
  expect_kind(fmt, 20, TD_MODE_2P, 1, r1, r2, 2048, 2);
  expect_kind(fmt, 20, TD_MODE_2P, 1, r1, r2, 4096, 1);
  expect_kind(fmt, 20, TD_MODE_2P, 1, r1, r2, 4097, 2);
  expect_kind(fmt, 20, TD_MODE_2P, 1, r1, r2, 32768, 2);
  expect_kind(fmt, 20, TD_MODE_2P, 1, r1, r2, 32769, 0);
  expect_kind(fmt, 20, TD_MODE_DEF, 1, r1, r2, 4097, 0);
  expect_kind(fmt, 20, TD_MODE_DEF, 0, r1, r2, 4097, 0);
  for (int mode = 0; mode < 3; ++mode) {
    expect_kind(fmt, 30, mode, 0, r1, r2, 40960, 2);
    expect_kind(fmt, 30, mode, 0, r1, r2, 40961, 0);
  }
}

}  // namespace

int main() {
  const int F32 = TD_OBS_F32, F16 = TD_OBS_F16;
  const int r1 = 8192, r2 = 4096;
  // float32, L 10, TD-def, single action: small2 again at every batch above one round
  const int def_single[][2] = {{1, 2}, {4096, 2}, {4097, 1}, {8192, 1}, {8193, 2}, {65536, 2}, {1048576, 2}};
  for (const auto& c : def_single) expect_kind(F32, 10, TD_MODE_DEF, 0, r1, r2, c[0], c[1]);
  // TD-atk and TD-2p, single action: up to three rounds
  for (int mode : {(int)TD_MODE_ATK, (int)TD_MODE_2P}) {
    expect_kind(F32, 10, mode, 0, r1, r2, 8193, 2);
    expect_kind(F32, 10, mode, 0, r1, r2, 24576, 2);
    expect_kind(F32, 10, mode, 0, r1, r2, 24577, 0);
  }
  // TD-def, multi-action: the large kernel above one round
  expect_kind(F32, 10, TD_MODE_DEF, 1, r1, r2, 4096, 2);
  expect_kind(F32, 10, TD_MODE_DEF, 1, r1, r2, 8192, 1);
  expect_kind(F32, 10, TD_MODE_DEF, 1, r1, r2, 8193, 0);
  rows_L20_L30(F32);
  // float16, L 10: every mode, single and multi-action (TD-atk has no multi-action handle)
  for (int mode = 0; mode < 3; ++mode)
    for (int multi = 0; multi < (mode == TD_MODE_ATK ? 1 : 2); ++multi) {
      expect_kind(F16, 10, mode, multi, r1, r2, 4096, 2);
      expect_kind(F16, 10, mode, multi, r1, r2, 4097, 1);
      expect_kind(F16, 10, mode, multi, r1, r2, 65536, 1);
    }
  // float16, L 20 / 30: the float32 rule on the residents it is given
  rows_L20_L30(F16);
  // a generic L has no small kernel: no resident boards, the large kernel at every batch
  for (int fmt : {F32, F16})
    for (int mode = 0; mode < 3; ++mode)
      for (int B : {1, 4096, 8192, 65536, 1048576}) expect_kind(fmt, 12, mode, 0, 0, 0, B, 0);
  // write-through: kind != 0 and B * 45 * L^2 * element <= 192 MiB
  for (int fmt : {F32, F16})
    for (int B : {1, 4096, 8192, 11184, 65536}) expect_wt(fmt, 10, 0, B, 0);
  for (int kind : {1, 2}) {
    expect_wt(F32, 10, kind, 11184, 1);
    expect_wt(F32, 10, kind, 11185, 0);
    expect_wt(F16, 10, kind, 16384, 1);
    expect_wt(F16, 10, kind, 22369, 1);
    expect_wt(F16, 10, kind, 22370, 0);
  }
  if (g_bad) return 1;
  std::printf("kernel_choice: %d cases ok\n", g_cases);
  return 0;
}
