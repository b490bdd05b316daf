// copy_check_host.cpp -- td_copy_boards' index validation (gym-td_amd/csrc/td_copy_check.h) on
// hand-made arrays, as a host program of its own: no HIP, no Python, no GPU.  Built with the
// address and undefined-behaviour sanitizers it shows that the check reads src[0..n) and
// dst[0..n) only, never indexes its scratch with an unchecked id, and leaves the scratch zero:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o copy_check_host scripts/copy_check_host.cpp && ./copy_check_host
//
// Every array is heap memory of exactly n ids, so a read past the end is a sanitizer report.
// Prints "copy_check: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../gym-td_amd/csrc/td_copy_check.h"

namespace {

int g_cases = 0, g_bad = 0;
std::vector<uint8_t> g_role;

void expect(const char* what, int B, const std::vector<int32_t>& s, const std::vector<int32_t>& d, int n, int want,
            bool null_src = false, bool null_dst = false) {
  // exact-size heap copies (an empty vector's data() may be NULL: keep one-past semantics out of it)
  int32_t* sp = null_src ? nullptr : new int32_t[s.size() ? s.size() : 1];
  int32_t* dp = null_dst ? nullptr : new int32_t[d.size() ? d.size() : 1];
  if (sp && !s.empty()) std::memcpy(sp, s.data(), s.size() * sizeof(int32_t));
  if (dp && !d.empty()) std::memcpy(dp, d.data(), d.size() * sizeof(int32_t));
  char msg[200] = "";
  const int got = td::copy_check(sp, dp, n, B, g_role, msg, sizeof msg);
  ++g_cases;
  bool ok = got == want && (want == td::COPY_OK ? msg[0] == 0 : msg[0] != 0);
  for (uint8_t r : g_role) ok = ok && r == 0;  // the scratch is clean again, refused or not
  if (!ok) {
    ++g_bad;
    std::printf("FAIL %s: got %d want %d msg '%s'\n", what, got, want, msg);
  }
  delete[] sp;
  delete[] dp;
}

}  // namespace

int main() {
  using namespace td;
  const int B = 8;
  expect("n = 0, NULL arrays", B, {}, {}, 0, COPY_OK, true, true);
  expect("n = 0, arrays", B, {}, {}, 0, COPY_OK);
  expect("n = -1", B, {}, {}, -1, COPY_BAD_COUNT);
  expect("n = INT_MIN", B, {}, {}, -2147483647 - 1, COPY_BAD_COUNT, true, true);
  expect("n = B + 1", B, {0, 0, 0, 0, 0, 0, 0, 0, 0}, {1, 2, 3, 4, 5, 6, 7, 1, 2}, B + 1, COPY_BAD_COUNT);
  expect("n = INT_MAX", B, {0}, {1}, 2147483647, COPY_BAD_COUNT);
  expect("NULL src", B, {}, {1}, 1, COPY_NULL, true, false);
  expect("NULL dst", B, {0}, {}, 1, COPY_NULL, false, true);
  expect("one pair", B, {0}, {1}, 1, COPY_OK);
  expect("fan-out from one root", B, {0, 0, 0, 0, 0, 0, 0}, {1, 2, 3, 4, 5, 6, 7}, 7, COPY_OK);
  expect("half to half", B, {0, 1, 2, 3}, {4, 5, 6, 7}, 4, COPY_OK);
  expect("last ids", B, {7, 7}, {0, 6}, 2, COPY_OK);
  // n = B: no split of B boards into B destinations leaves a source, so every such call is refused
  expect("n = B", B, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7}, B, COPY_OVERLAP);
  expect("n = B, dst twice first", B, {0, 0, 0, 0, 0, 0, 0, 0}, {1, 1, 2, 3, 4, 5, 6, 7}, B, COPY_DST_TWICE);
  expect("src = -1", B, {-1}, {1}, 1, COPY_RANGE);
  expect("src = B", B, {B}, {1}, 1, COPY_RANGE);
  expect("dst = -1", B, {0}, {-1}, 1, COPY_RANGE);
  expect("dst = B", B, {0}, {B}, 1, COPY_RANGE);
  expect("dst = INT_MAX", B, {0, 1}, {2, 2147483647}, 2, COPY_RANGE);
  expect("src = INT_MIN after good pairs", B, {0, 1, -2147483647 - 1}, {2, 3, 4}, 3, COPY_RANGE);
  expect("dst twice", B, {0, 1, 2}, {5, 6, 5}, 3, COPY_DST_TWICE);
  expect("dst twice, adjacent", B, {0, 0}, {3, 3}, 2, COPY_DST_TWICE);
  expect("self copy", B, {2}, {2}, 1, COPY_OVERLAP);
  expect("overlap, source later", B, {0, 1}, {1, 2}, 2, COPY_OVERLAP);
  expect("overlap, source earlier", B, {1, 0}, {2, 1}, 2, COPY_OVERLAP);
  expect("swap", B, {0, 1}, {1, 0}, 2, COPY_OVERLAP);
  expect("range wins over duplicates", B, {0, 0, 9}, {1, 1, 2}, 3, COPY_RANGE);
  // one board, and a scratch vector of another size from the handle before it
  expect("B = 1, n = 1", 1, {0}, {0}, 1, COPY_OVERLAP);
  expect("B = 1, n = 0", 1, {}, {}, 0, COPY_OK);
  expect("B = 1, id 1", 1, {0}, {1}, 1, COPY_RANGE);
  expect("B = 70000, far ids", 70000, {69999, 0}, {1, 69998}, 2, COPY_OK);
  expect("B = 70000, dst twice far", 70000, {0, 0}, {69999, 69999}, 2, COPY_DST_TWICE);
  if (g_bad) return 1;
  std::printf("copy_check: %d cases ok\n", g_cases);
  return 0;
}
