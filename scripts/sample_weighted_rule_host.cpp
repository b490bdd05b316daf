// sample_weighted_rule_host.cpp -- the rule of td_sample_weighted (gym-td_amd/csrc/td_sample.h:
// sample_quant, sample_threshold, sample_pick_weighted) and what the call refuses of its io
// (td_call_check.h sample_w_io_refused), verdict and whole message in refusal order, as a host
// program of its own: no HIP, no Python, no GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o sample_weighted_rule_host scripts/sample_weighted_rule_host.cpp && ./sample_weighted_rule_host
//
// Every array is heap memory of exactly the size passed.  With arguments "word m0 m1 ..." (decimal
// or 0x...) it prints "pick m S" of that row instead, and with "q bits" the quantised value of the
// float32 with those bits, for the Python mirror's test.
// Prints "sample_weighted_rule: N cases ok" and returns 0, or names the first case that went wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../gym-td_amd/csrc/td_call_check.h"
#include "../gym-td_amd/csrc/td_sample.h"

namespace {

int g_cases = 0, g_bad = 0;
const size_t kCap = 240;

void verdict(const char* what, bool ok, const char* msg) {
  ++g_cases;
  if (!ok && !g_bad++) std::printf("FAIL %s: '%s'\n", what, msg);
}

void expect_q(const char* what, float w, uint32_t want) {
  char buf[64];
  const uint32_t q = td::sample_quant(w);
  std::snprintf(buf, sizeof buf, "%u, not %u", q, want);
  verdict(what, q == want, buf);
}

void expect_pick(const char* what, const std::vector<uint32_t>& row, uint64_t word, int want, uint64_t want_m,
                 uint64_t want_S) {
  uint32_t* m = new uint32_t[row.size()];
  std::memcpy(m, row.data(), row.size() * sizeof(uint32_t));
  uint64_t* mass = new uint64_t[2];
  const int pick = td::sample_pick_weighted(m, (int)row.size(), word, mass);
  char buf[96];
  std::snprintf(buf, sizeof buf, "pick %d mass (%llu, %llu)", pick, (unsigned long long)mass[0], (unsigned long long)mass[1]);
  verdict(what, pick == want && mass[0] == want_m && mass[1] == want_S &&
                    td::sample_pick_weighted(m, (int)row.size(), word, nullptr) == want, buf);
  delete[] mass;
  delete[] m;
}

const unsigned kSize = 80;  // sizeof(td_sample_w_io)
const int kAbi = 3;
const size_t kMaxPitch = 65536, kRow = 601;

void expect_io(const char* fn, const td::SampleWIoSeen& v, const std::string& want) {
  char* msg = new char[kCap];
  std::memset(msg, '#', kCap);
  msg[kCap - 1] = 0;
  const bool refused = td::sample_w_io_refused(fn, v, kSize, kAbi, kMaxPitch, msg, kCap);
  verdict(fn, refused == !want.empty() && (refused ? want == msg : msg[0] == '#'), msg);
  delete[] msg;
}

// an io that is accepted: both sides of TD-2p with weights and masses
td::SampleWIoSeen full(int mode) {
  td::SampleWIoSeen v;
  v.io = true; v.size = kSize; v.abi = kAbi; v.handle = true; v.mode = mode; v.row = kRow;
  if (mode != 1) v.def_act = v.def_w = v.def_mass = true;
  if (mode != 0) v.atk_act = v.atk_w = v.atk_mass = true;
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  using namespace td;
  if (argc == 3 && !std::strcmp(argv[1], "q")) {
    const uint32_t bits = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    float w;
    std::memcpy(&w, &bits, 4);
    std::printf("%u\n", sample_quant(w));
    return 0;
  }
  if (argc >= 3) {
    std::vector<uint32_t> row;
    for (int i = 2; i < argc; ++i) row.push_back((uint32_t)std::strtoull(argv[i], nullptr, 0));
    uint64_t mass[2];
    const int pick = sample_pick_weighted(row.data(), (int)row.size(), std::strtoull(argv[1], nullptr, 0), mass);
    std::printf("%d %llu %llu\n", pick, (unsigned long long)mass[0], (unsigned long long)mass[1]);
    return 0;
  }

  // the quantiser's edges
  const float inf = std::numeric_limits<float>::infinity();
  expect_q("0", 0.0f, 0u);
  expect_q("-0", -0.0f, 0u);
  expect_q("-1", -1.0f, 0u);
  expect_q("NaN", std::numeric_limits<float>::quiet_NaN(), 0u);
  expect_q("-inf", -inf, 0u);
  expect_q("+inf", inf, 2147483648u);
  expect_q("2.0", 2.0f, 2147483648u);
  expect_q("1.0", 1.0f, 2147483648u);
  expect_q("below 1", std::nextafterf(1.0f, 0.0f), 2147483520u);  // (1 - 2^-24) 2^31 = 2^31 - 2^7
  expect_q("0.5", 0.5f, 1073741824u);
  expect_q("0.3f", 0.3f, 644245120u);  // 0x3E99999A = 10066330 * 2^-25
  expect_q("2^-31", std::ldexp(1.0f, -31), 1u);
  expect_q("below 2^-31", std::nextafterf(std::ldexp(1.0f, -31), 0.0f), 0u);
  expect_q("3 * 2^-31", std::ldexp(3.0f, -31), 3u);
  expect_q("subnormal", std::numeric_limits<float>::denorm_min() * 1000.0f, 0u);
  expect_q("min normal", std::numeric_limits<float>::min(), 0u);

  // the threshold: floor(word * S / 2^64)
  verdict("r word 0", sample_threshold(0, 12345) == 0, "");
  verdict("r word max", sample_threshold(~0ull, 1ull << 44) == (1ull << 44) - 1, "");
  verdict("r half", sample_threshold(1ull << 63, 7) == 3, "");
  verdict("r S = 1", sample_threshold(~0ull, 1) == 0, "");

  // known answers, computed independently (tests/test_sample_weighted_ref.py holds the same rows)
  const std::vector<uint32_t> A = {3u, 0u, 5u, 2147483648u, 1u};  // S = 2^31 + 9
  expect_pick("A word 0", A, 0, 0, 3, 2147483657ull);
  expect_pick("A word max", A, ~0ull, 4, 1, 2147483657ull);
  expect_pick("A half", A, 1ull << 63, 3, 2147483648ull, 2147483657ull);      // r = 2^30 + 4
  expect_pick("A r = 0", A, 0x00000000EFFFFFFFull, 0, 3, 2147483657ull);       // word * S < 2^64
  expect_pick("A r = 3", A, 0x0000000600000000ull, 2, 5, 2147483657ull);       // 3 * 2^64 + 27 * 2^33: 3 > 3 fails, 8 > 3
  expect_pick("zero", {0u, 0u, 0u}, 0x123456789ABCDEFull, 2, 0, 0);            // S == 0: the last entry, (0, 0)
  expect_pick("one-hot", {0u, 0u, 77u, 0u}, ~0ull, 2, 77, 77);
  expect_pick("one-hot 0", {0u, 0u, 77u, 0u}, 0, 2, 77, 77);
  expect_pick("last only", {0u, 0u, 0u, 9u}, 1ull << 62, 3, 9, 9);
  {  // S near 2^44: 6,145 entries of 2^31 (a 32 x 32 board's row, all legal, all weight 1)
    const std::vector<uint32_t> B(6145, 2147483648u);
    const uint64_t S = 6145ull << 31;
    expect_pick("B word max", B, ~0ull, 6144, 2147483648ull, S);   // r = S - 1
    expect_pick("B half", B, 1ull << 63, 3072, 2147483648ull, S);  // r = 6145 * 2^30: (e + 1) 2^31 > r from e = 3072
    expect_pick("B word 0", B, 0, 0, 2147483648ull, S);
    std::vector<uint32_t> C = B;  // 8,192 entries: S = 2^44 exactly
    C.resize(8192, 2147483648u);
    expect_pick("C word max", C, ~0ull, 8191, 2147483648ull, 1ull << 44);
    expect_pick("C r = 2^44 - 2", C, ~0ull - (1ull << 20), 8191, 2147483648ull, 1ull << 44);
    expect_pick("C r = 2^44 - 2^32", C, 0xFFF0000000000000ull, 8190, 2147483648ull, 1ull << 44);  // 8190 * 2^31 > r fails
  }

  for (const char* fn : {"td_sample_weighted", "td_sample_weighted_boards", "td_sample_weighted_boards_dev"}) {
    const std::string f = fn;
    SampleWIoSeen v;  // a NULL io wins over a NULL handle
    expect_io(fn, v, f + ": NULL io");
    v.io = true; v.size = kSize - 8; v.abi = kAbi;  // a bad header wins over a NULL handle
    expect_io(fn, v, f + ": td_sample_w_io has size 72 / abi 3, this library expects size 80 / abi 3 (call td_sample_w_io_init)");
    v.size = kSize; v.abi = 2; v.handle = true;
    expect_io(fn, v, f + ": td_sample_w_io has size 80 / abi 2, this library expects size 80 / abi 3 (call td_sample_w_io_init)");
    v.abi = kAbi; v.handle = false;
    expect_io(fn, v, f + ": NULL handle");
    v.handle = true; v.def_w = v.atk_w = v.def_mass = true;  // weights and masses alone are no action output
    expect_io(fn, v, f + ": no action output wanted (def_act and atk_act are NULL)");
    // a side the mode lacks: any of its pointers, and before a missing weight
    const std::string no_def = f + ": TD-atk has no defender side (def_act / def_w / def_mass)";
    const std::string no_atk = f + ": TD-def has no attacker side (atk_act / atk_w / atk_mass)";
    for (int p = 0; p < 3; ++p) {
      SampleWIoSeen a = full(1), d = full(0);
      a.atk_w = false; d.def_w = false;
      (p == 0 ? a.def_act : p == 1 ? a.def_w : a.def_mass) = true;
      (p == 0 ? d.atk_act : p == 1 ? d.atk_w : d.atk_mass) = true;
      expect_io(fn, a, no_def);
      expect_io(fn, d, no_atk);
    }
    {  // an action without its weights, a mass without its action; before the alignment
      SampleWIoSeen x = full(2);
      x.def_w = false; x.atk_w_aligned = false;
      expect_io(fn, x, f + ": def_act without its weights (def_w is NULL)");
      x = full(2); x.atk_w = false; x.def_w_aligned = false;
      expect_io(fn, x, f + ": atk_act without its weights (atk_w is NULL)");
      x = full(2); x.def_act = false; x.pitch = 1;
      expect_io(fn, x, f + ": def_mass without its action (def_act is NULL)");
      x = full(2); x.atk_act = false; x.pitch = 1;
      expect_io(fn, x, f + ": atk_mass without its action (atk_act is NULL)");
    }
    {  // alignment before the pitch, the pitch before multi-action
      SampleWIoSeen x = full(2);
      x.def_w_aligned = false; x.pitch = 600;
      expect_io(fn, x, f + ": def_w is no multiple of 4 (float32 rows)");
      x = full(2); x.atk_w_aligned = false; x.multi = 1;
      expect_io(fn, x, f + ": atk_w is no multiple of 4 (float32 rows)");
      x = full(2); x.pitch = 600; x.multi = 1;
      expect_io(fn, x, f + ": def_w_pitch 600 outside [601, 65536] (6 L^2 + 1 floats per row)");
      x.pitch = 65537;
      expect_io(fn, x, f + ": def_w_pitch 65537 outside [601, 65536] (6 L^2 + 1 floats per row)");
      x.pitch = 601;
      expect_io(fn, x, f + ": the defender side is not supported with multi-action (one discrete action is sampled); "
                           "the attacker side is");
    }
    // accepted
    expect_io(fn, full(0), "");
    expect_io(fn, full(1), "");
    expect_io(fn, full(2), "");
    for (size_t pitch : {(size_t)0, kRow, (size_t)604, kMaxPitch}) {
      SampleWIoSeen x = full(2);
      x.pitch = pitch;
      expect_io(fn, x, "");
    }
    {
      SampleWIoSeen x = full(2);  // the attacker side of a multi-action handle; a pitch without the defender is not looked at
      x.multi = 1; x.def_act = x.def_mass = false; x.pitch = 5;
      expect_io(fn, x, "");
      x = full(2); x.def_mass = x.atk_mass = false;  // no masses
      expect_io(fn, x, "");
      x = full(2); x.atk_act = x.atk_mass = false;   // weights without their action are not looked at
      expect_io(fn, x, "");
    }
  }
  if (g_bad) return 1;
  std::printf("sample_weighted_rule: %d cases ok\n", g_cases);
  return 0;
}
