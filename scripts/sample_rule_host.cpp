// sample_rule_host.cpp -- the rule of td_sample_actions (gym-td_amd/csrc/td_sample.h) and what the
// call refuses of its io (td_call_check.h sample_io_refused), verdict and whole message, as a
// host program of its own: no HIP, no Python, no GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o sample_rule_host scripts/sample_rule_host.cpp && ./sample_rule_host
//
// Every message buffer is heap memory of exactly the size passed; an accepted io leaves it
// untouched.  With arguments "seed ticket b j" (decimal or 0x...) it prints that draw's word
// and u instead, for the Python mirror's test.
// Prints "sample_rule: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../gym-td_amd/csrc/td_call_check.h"
#include "../gym-td_amd/csrc/td_sample.h"

namespace {

int g_cases = 0, g_bad = 0;
const size_t kCap = 240;

void verdict(const char* what, bool ok, const char* msg) {
  ++g_cases;
  if (!ok && !g_bad++) std::printf("FAIL %s: '%s'\n", what, msg);
}

void expect_word(uint64_t seed, uint64_t ticket, uint64_t b, int j, uint64_t want_word, uint32_t want_u) {
  const uint64_t w = td::sample_word(seed, ticket, b, j);
  const uint32_t u = td::sample_u(td::sample_key(seed, ticket), b, j);
  char buf[64];
  std::snprintf(buf, sizeof buf, "0x%016llX / %u", (unsigned long long)w, u);
  verdict("word", w == want_word && u == want_u && u == (uint32_t)(w >> 32), buf);
}

const unsigned kSize = 64;  // sizeof(td_sample_io)
const int kAbi = 3;

void expect_io(const char* fn, const td::SampleIoSeen& v, const std::string& want) {
  char* msg = new char[kCap];
  std::memset(msg, '#', kCap);
  msg[kCap - 1] = 0;
  const bool refused = td::sample_io_refused(fn, v, kSize, kAbi, msg, kCap);
  verdict(fn, refused == !want.empty() && (refused ? want == msg : msg[0] == '#'), msg);
  delete[] msg;
}

td::SampleIoSeen seen(int mode, bool da, bool aa, bool dc, bool ac) {
  td::SampleIoSeen v;
  v.io = true; v.size = kSize; v.abi = kAbi; v.handle = true; v.mode = mode;
  v.def_act = da; v.atk_act = aa; v.def_count = dc; v.atk_count = ac;
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  using namespace td;
  if (argc == 5) {
    const uint64_t w = sample_word(std::strtoull(argv[1], nullptr, 0), std::strtoull(argv[2], nullptr, 0),
                                   std::strtoull(argv[3], nullptr, 0), std::atoi(argv[4]));
    std::printf("0x%016llX %u\n", (unsigned long long)w, (unsigned)(w >> 32));
    return 0;
  }
  // splitmix64's published first output, and the five known answers
  verdict("sm(0)", sample_sm(0) == 0xE220A8397B1DCDAFull, "sm(0)");
  expect_word(0, 0, 0, 0, 0x238275BC38FCBE91ull, 595752380u);
  expect_word(0, 0, 0, 1, 0x421DAF3033E887A3ull, 1109241648u);
  expect_word(1, 2, 3, 1, 0xB39B489899B5598Aull, 3013298328u);
  expect_word(0xDEADBEEFCAFEF00Dull, ~0ull, 65535, 3, 0x72FF560395D91BD3ull, 1929336323u);
  expect_word(2026, 7, 2099, 2, 0x7904480F124E732Bull, 2030323727u);
  // the choice: idle iff nothing is legal or u < idle; the pick stays inside [0, n) at both ends of u
  verdict("idle n = 0", sample_idles(0xffffffffu, 0u, 0), "");
  verdict("idle 0 never", !sample_idles(0u, 0u, 1), "");
  verdict("idle below", sample_idles(5u, 6u, 3) && !sample_idles(6u, 6u, 3), "");
  verdict("idle max", sample_idles(0xfffffffeu, 0xffffffffu, 1) && !sample_idles(0xffffffffu, 0xffffffffu, 1), "");
  for (int n : {1, 2, 7, 301, 600, 6144})
    verdict("pick ends", sample_pick(0u, n) == 0 && sample_pick(0xffffffffu, n) == n - 1, "");
  verdict("pick middle", sample_pick(0x80000000u, 7) == 3 && sample_pick(0x40000000u, 600) == 150, "");

  for (const char* fn : {"td_sample_actions", "td_sample_actions_boards", "td_sample_actions_boards_dev"}) {
    const std::string f = fn;
    SampleIoSeen v;  // a NULL io wins over a NULL handle
    expect_io(fn, v, f + ": NULL io");
    v.io = true; v.size = kSize - 8; v.abi = kAbi;  // a bad header wins over a NULL handle
    expect_io(fn, v, f + ": td_sample_io has size 56 / abi 3, this library expects size 64 / abi 3 (call td_sample_io_init)");
    v.size = kSize; v.abi = 2; v.handle = true;
    expect_io(fn, v, f + ": td_sample_io has size 64 / abi 2, this library expects size 64 / abi 3 (call td_sample_io_init)");
    v.abi = kAbi; v.handle = false;
    expect_io(fn, v, f + ": NULL handle");
    for (int mode = 0; mode < 3; ++mode) {  // counts alone are no action output
      expect_io(fn, seen(mode, false, false, false, false), f + ": no action output wanted (def_act and atk_act are NULL)");
      expect_io(fn, seen(mode, false, false, true, true), f + ": no action output wanted (def_act and atk_act are NULL)");
    }
    const std::string no_def = f + ": TD-atk has no defender side (def_act / def_count)";
    const std::string no_atk = f + ": TD-def has no attacker side (atk_act / atk_count)";
    expect_io(fn, seen(1, true, true, false, false), no_def);
    expect_io(fn, seen(1, false, true, true, false), no_def);
    expect_io(fn, seen(0, true, true, false, false), no_atk);
    expect_io(fn, seen(0, true, false, false, true), no_atk);
    // accepted
    expect_io(fn, seen(0, true, false, false, false), "");
    expect_io(fn, seen(0, true, false, true, false), "");
    expect_io(fn, seen(1, false, true, false, true), "");
    expect_io(fn, seen(2, true, true, true, true), "");
    expect_io(fn, seen(2, true, false, false, false), "");
    expect_io(fn, seen(2, false, true, true, false), "");
  }
  if (g_bad) return 1;
  std::printf("sample_rule: %d cases ok\n", g_cases);
  return 0;
}
