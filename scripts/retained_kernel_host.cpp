// retained_kernel_host.cpp -- the kind of a skipping launch (gym-td_amd/csrc/td_kernel_choice.h
// retained_kernel_kind) at every boundary of its table, the order in which a handle's two
// kinds are resolved (KernelChoice::resolve: forced versus TD_KERNEL_AUTO), and what the two
// kernel-kind setters do to the record (KernelChoice::force_both, force_retained, kernel_kind_ok),
// as a host program of its own: no HIP, no Python, no GPU.  The rule decides which kernel the bench's timed steps run; a
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
#include <cstring>
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
  td::KernelChoice k;  // forced as the setters leave it: the flag, and the kind in its place
  k.kernel_forced = ff >= 0;
  k.retained_forced = fr >= 0;
  if (ff >= 0) k.small = ff;
  if (fr >= 0) k.small_retained = fr;
  k.resolve(L, mode, multi, fmt, B, r1, r2);
  ++g_cases;
  const bool wt_ok = k.obs_wt == td::obs_write_through(k.small, L, fmt, B) &&
                     k.obs_wt_retained == td::obs_write_through(k.small_retained, L, fmt, B) && k.name_kind == k.small &&
                     k.kind(0) == k.small && k.kind(1) == k.small_retained && k.write_through(0) == k.obs_wt &&
                     k.write_through(1) == k.obs_wt_retained;
  if ((k.small != want_full || k.small_retained != want_retained || !wt_ok) && !g_bad++)
    std::printf("FAIL kinds: forced %d / %d %s L %d %s %s B %d: got %d / %d want %d / %d (flags ok %d)\n", ff, fr,
                fmt ? "float16" : "float32", L, kModes[mode], multi ? "multi-action" : "single action", B, k.small,
                k.small_retained, want_full, want_retained, (int)wt_ok);
}

// One step of a setter sequence on a TD-def 10x10 handle of 65,536 boards (rules: small2 / small):
// the setter, then the resolve td_capi.hip's apply_kernel runs behind it.
struct Seq {
  td::KernelChoice k;
  int fmt = TD_OBS_F32;
  void resolve() { k.resolve(10, TD_MODE_DEF, 0, fmt, 65536, 8192, 4096); }
  void both(int kind) { k.force_both(kind); resolve(); }
  void retained(int kind) { k.force_retained(kind); resolve(); }
  void format(int f) { fmt = f; resolve(); }
  void expect(const char* what, int full, int ret, int forced, int ret_forced) {
    ++g_cases;
    if ((k.small != full || k.small_retained != ret || k.kernel_forced != forced || k.retained_forced != ret_forced ||
         k.name_kind != full) && !g_bad++)
      std::printf("FAIL sequence, %s: kinds %d / %d forced %d / %d name %d, want %d / %d forced %d / %d\n", what, k.small,
                  k.small_retained, k.kernel_forced, k.retained_forced, k.name_kind, full, ret, forced, ret_forced);
  }
};

void expect_kind_ok(const char* fn, int kind, int L, const char* want) {
  char msg[200] = "";
  const bool ok = td::kernel_kind_ok(fn, kind, L, msg, sizeof msg);
  ++g_cases;
  if ((ok != (want[0] == 0) || std::strcmp(msg, want) != 0) && !g_bad++)
    std::printf("FAIL kernel_kind_ok %s kind %d L %d: got %d '%s' want '%s'\n", fn, kind, L, (int)ok, msg, want);
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

  // ---- the setters (kinds as the ABI numbers them: TD_KERNEL_AUTO 0, LARGE 1, SMALL 2, SMALL2 3)
  {
    Seq q;
    q.resolve();
    q.expect("as created", 2, 1, 0, 0);
    // a forced kind survives a format change, for both kinds of launch
    q.both(TD_KERNEL_LARGE);
    q.expect("td_set_step_kernel(large)", 0, 0, 1, 1);
    q.format(F16);
    q.expect("forced large, then float16", 0, 0, 1, 1);
    q.format(F32);
    q.expect("forced large, float32 again", 0, 0, 1, 1);
    // TD_KERNEL_AUTO gives both back to their rules, in the format of the moment
    q.both(TD_KERNEL_AUTO);
    q.expect("td_set_step_kernel(auto)", 2, 1, 0, 0);
    q.format(F16);
    q.expect("auto, then float16", 1, 1, 0, 0);
    q.format(F32);
    q.expect("auto, float32 again", 2, 1, 0, 0);
    // the retained setter leaves the full kind alone, forced or not
    q.retained(TD_KERNEL_SMALL2);
    q.expect("td_set_retained_step_kernel(small2)", 2, 2, 0, 1);
    q.format(F16);
    q.expect("retained small2 survives float16; the full kind follows its rule", 1, 2, 0, 1);
    q.format(F32);
    q.retained(TD_KERNEL_LARGE);
    q.expect("td_set_retained_step_kernel(large)", 2, 0, 0, 1);
    q.retained(TD_KERNEL_AUTO);
    q.expect("td_set_retained_step_kernel(auto)", 2, 1, 0, 0);
    q.both(TD_KERNEL_SMALL);
    q.retained(TD_KERNEL_SMALL2);
    q.expect("full forced small, retained forced small2", 1, 2, 1, 1);
    q.retained(TD_KERNEL_AUTO);
    q.expect("retained back to its rule on a forced full kind: the full kind stays forced", 1, 1, 1, 0);
    q.both(TD_KERNEL_LARGE);
    q.retained(TD_KERNEL_AUTO);
    q.expect("the rule on a forced large kind", 0, 1, 1, 0);
    q.both(TD_KERNEL_AUTO);
    q.expect("td_set_step_kernel(auto) takes a forced retained kind back too", 2, 1, 0, 0);
  }
  // the kind / map-side check, with the caller's name; an unknown kind wins over the map side
  for (const char* fn : {"td_set_step_kernel", "td_set_retained_step_kernel"}) {
    char want[200];
    for (int L : {10, 20, 30, 12})
      for (int kind : {0, 1}) expect_kind_ok(fn, kind, L, "");
    for (int L : {10, 20, 30})
      for (int kind : {2, 3}) expect_kind_ok(fn, kind, L, "");
    for (int L : {4, 12, 32})
      for (int kind : {2, 3}) {
        std::snprintf(want, sizeof want, "%s: L = %d has no small-batch step kernel (only L = 10 / 20 / 30)", fn, L);
        expect_kind_ok(fn, kind, L, want);
      }
    for (int L : {10, 12})
      for (int kind : {-1, 4, -2147483647 - 1}) {
        std::snprintf(want, sizeof want, "%s: unknown kernel kind %d", fn, kind);
        expect_kind_ok(fn, kind, L, want);
      }
  }
  if (g_bad) return 1;
  std::printf("retained_kernel: %d cases ok\n", g_cases);
  return 0;
}
