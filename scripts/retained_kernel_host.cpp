// retained_kernel_host.cpp -- the kind of a skipping launch (gym-td_amd/csrc/td_kernel_choice.h
// retained_kernel_kind) at every boundary of its table, and the order in which a handle's two
// kinds are resolved (resolve_step_kinds: forced versus TD_KERNEL_AUTO), as a host program of its
// own: no HIP, no Python, no GPU.  The rule decides which kernel the bench's timed steps run; a
// boundary one board off would pass every parity test and show only as a slower step.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o retained_kernel_host scripts/retained_kernel_host.cpp && ./retained_kernel_host
//
// Kinds: 0 large, 1 small, 2 small2; -1 where a forced kind is asked for means TD_KERNEL_AUTO.  The
// resident counts are inputs of the rule: 8,192 boards with one wave each and 4,096 with two at
// L = 10 (256 CUs x 4 SIMDs x 8 waves), half of them at L = 20 / 30.
// Prints "retained_kernel: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <initializer_list>

#define __host__
#define __device__
#include "../gym-td_amd/csrc/td_kernel_choice.h"

namespace {

int g_cases = 0, g_bad = 0;
const char* kModes[3] = {"TD-def", "TD-atk", "TD-2p"};
const int F32 = TD_OBS_F32, F16 = TD_OBS_F16;

void expect_retained(int fmt, int L, int mode, int multi, int r1, int r2, int B, int full, int want) {
  const int got = td::retained_kernel_kind(L, mode, multi, fmt, B, r1, r2, full);
  ++g_cases;
  if (got != want && !g_bad++)
    std::printf("FAIL retained kind: %s L %d %s %s residents %d / %d B %d full %d: got %d want %d\n",
                fmt ? "float16" : "float32", L, kModes[mode], multi ? "multi-action" : "single action", r1, r2, B, full,
                got, want);
}

void expect_kinds(int ff, int fr, int fmt, int L, int mode, int multi, int r1, int r2, int B, int want_full,
                  int want_retained) {
  const td::StepKinds k = td::resolve_step_kinds(ff, fr, L, mode, multi, fmt, B, r1, r2);
  ++g_cases;
  if ((k.full != want_full || k.retained != want_retained) && !g_bad++)
    std::printf("FAIL kinds: forced %d / %d %s L %d %s %s B %d: got %d / %d want %d / %d\n", ff, fr,
                fmt ? "float16" : "float32", L, kModes[mode], multi ? "multi-action" : "single action", B, k.full,
                k.retained, want_full, want_retained);
}

}  // namespace

int main() {
  const int r1 = 8192, r2 = 4096;
  // float32, L 10: the full kind up to one round of boards, the small kernel above -- every mode,
  // single and multi-action (TD-atk has no multi-action handle), whatever the full kind is
  for (int mode = 0; mode < 3; ++mode)
    for (int multi = 0; multi < (mode == TD_MODE_ATK ? 1 : 2); ++multi)
      for (int full = 0; full < 3; ++full) {
        for (int B : {1, 4096, 4097, 8191, 8192}) expect_retained(F32, 10, mode, multi, r1, r2, B, full, full);
        for (int B : {8193, 8256, 12288, 16384, 24576, 24577, 65536, 1048576})
          expect_retained(F32, 10, mode, multi, r1, r2, B, full, 1);
      }
  // the boundary is the resident count the handle measured, not 8,192
  expect_retained(F32, 10, TD_MODE_DEF, 0, 7168, 3584, 7168, 2, 2);
  expect_retained(F32, 10, TD_MODE_DEF, 0, 7168, 3584, 7169, 2, 1);
  // float16 at L 10, and L 20 / 30 in both formats: the full kind at every batch
  for (int full = 0; full < 3; ++full)
    for (int B : {1, 4096, 8192, 8193, 16384, 65536}) {
      for (int mode = 0; mode < 3; ++mode) expect_retained(F16, 10, mode, 0, r1, r2, B, full, full);
      for (int fmt : {F32, F16}) {
        expect_retained(fmt, 20, TD_MODE_2P, 1, 4096, 2048, B, full, full);
        expect_retained(fmt, 20, TD_MODE_DEF, 0, 4096, 2048, B, full, full);
        expect_retained(fmt, 30, TD_MODE_DEF, 0, 4096, 2048, B, full, full);
      }
    }
  // a generic L has no small kernel: no resident boards, the full kind (the large kernel) at every batch
  for (int fmt : {F32, F16})
    for (int B : {1, 8192, 8193, 65536, 1048576}) expect_retained(fmt, 12, TD_MODE_DEF, 0, 0, 0, B, 0, 0);

  // ---- resolution order
  // TD_KERNEL_AUTO for both: the two rules.  TD-def 10x10: small2 / small above a round, the pinned
  // small2 for a launch that writes every window at 16,384 and 65,536 boards
  expect_kinds(-1, -1, F32, 10, TD_MODE_DEF, 0, r1, r2, 4096, 2, 2);
  expect_kinds(-1, -1, F32, 10, TD_MODE_DEF, 0, r1, r2, 8192, 1, 1);
  expect_kinds(-1, -1, F32, 10, TD_MODE_DEF, 0, r1, r2, 8256, 2, 1);
  expect_kinds(-1, -1, F32, 10, TD_MODE_DEF, 0, r1, r2, 16384, 2, 1);
  expect_kinds(-1, -1, F32, 10, TD_MODE_DEF, 0, r1, r2, 65536, 2, 1);
  // the other pairs the table produces: (large, small) where the full rule has gone over to large
  expect_kinds(-1, -1, F32, 10, TD_MODE_ATK, 0, r1, r2, 24576, 2, 1);
  expect_kinds(-1, -1, F32, 10, TD_MODE_ATK, 0, r1, r2, 24577, 0, 1);
  expect_kinds(-1, -1, F32, 10, TD_MODE_2P, 0, r1, r2, 65536, 0, 1);
  expect_kinds(-1, -1, F32, 10, TD_MODE_DEF, 1, r1, r2, 8193, 0, 1);
  expect_kinds(-1, -1, F32, 10, TD_MODE_2P, 1, r1, r2, 16384, 0, 1);
  // no change where the rule returns the full kind
  expect_kinds(-1, -1, F16, 10, TD_MODE_DEF, 0, r1, r2, 65536, 1, 1);
  expect_kinds(-1, -1, F32, 20, TD_MODE_2P, 1, 4096, 2048, 16384, 2, 2);
  expect_kinds(-1, -1, F32, 30, TD_MODE_DEF, 0, 4096, 2048, 16384, 2, 2);
  expect_kinds(-1, -1, F32, 30, TD_MODE_DEF, 0, 4096, 2048, 40961, 0, 0);
  expect_kinds(-1, -1, F32, 12, TD_MODE_DEF, 0, 0, 0, 65536, 0, 0);
  // td_set_step_kernel forces both kinds: every launch runs the forced kernel
  for (int k = 0; k < 3; ++k)
    for (int B : {64, 8192, 8193, 65536}) expect_kinds(k, k, F32, 10, TD_MODE_DEF, 0, r1, r2, B, k, k);
  // the retained kind alone forced: the full kind keeps its rule
  for (int k = 0; k < 3; ++k) {
    expect_kinds(-1, k, F32, 10, TD_MODE_DEF, 0, r1, r2, 65536, 2, k);
    expect_kinds(-1, k, F32, 10, TD_MODE_DEF, 0, r1, r2, 64, 2, k);
    expect_kinds(-1, k, F32, 30, TD_MODE_DEF, 0, 4096, 2048, 16384, 2, k);
  }
  // the full kind forced, the retained kind given back to its rule: the rule on the forced kind
  expect_kinds(0, -1, F32, 10, TD_MODE_DEF, 0, r1, r2, 65536, 0, 1);
  expect_kinds(2, -1, F32, 10, TD_MODE_DEF, 0, r1, r2, 65536, 2, 1);
  expect_kinds(0, -1, F32, 10, TD_MODE_DEF, 0, r1, r2, 8192, 0, 0);
  expect_kinds(0, -1, F32, 30, TD_MODE_DEF, 0, 4096, 2048, 16384, 0, 0);
  expect_kinds(0, -1, F16, 10, TD_MODE_DEF, 0, r1, r2, 65536, 0, 0);
  if (g_bad) return 1;
  std::printf("retained_kernel: %d cases ok\n", g_cases);
  return 0;
}
