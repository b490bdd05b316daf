// ids_check_host.cpp -- td_step_boards' board-list validation (gym-td_amd/csrc/td_ids_check.h)
// on hand-made lists, as a host program of its own: no HIP, no Python, no GPU.  Built with the
// address and undefined-behaviour sanitizers it shows that the check reads ids[0..n) only,
// never indexes its scratch with an unchecked id, and leaves the scratch zero:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o ids_check_host scripts/ids_check_host.cpp && ./ids_check_host
//
// Every list is heap memory of exactly its ids, so a read past the end is a sanitizer report.
// Prints "ids_check: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../gym-td_amd/csrc/td_ids_check.h"

namespace {

int g_cases = 0, g_bad = 0;
std::vector<uint8_t> g_seen;

void expect(const char* what, int B, const std::vector<int32_t>& ids, int n, int want, bool null_ids = false) {
  // an exact-size heap copy (an empty vector's data() may be NULL: keep one-past semantics out of it)
  int32_t* p = null_ids ? nullptr : new int32_t[ids.size() ? ids.size() : 1];
  if (p && !ids.empty()) std::memcpy(p, ids.data(), ids.size() * sizeof(int32_t));
  char msg[200] = "";
  const int got = td::ids_check(p, n, B, g_seen, msg, sizeof msg);
  ++g_cases;
  bool ok = got == want && (want == td::IDS_OK ? msg[0] == 0 : msg[0] != 0);
  for (uint8_t r : g_seen) ok = ok && r == 0;  // the scratch is clean again, refused or not
  if (!ok) {
    ++g_bad;
    std::printf("FAIL %s: got %d want %d msg '%s'\n", what, got, want, msg);
  }
  delete[] p;
}

}  // namespace

int main() {
  using namespace td;
  const int B = 8;
  expect("n = 0, NULL list", B, {}, 0, IDS_OK, true);
  expect("n = 0, a list", B, {}, 0, IDS_OK);
  expect("n = -1", B, {}, -1, IDS_BAD_COUNT);
  expect("n = INT_MIN", B, {}, -2147483647 - 1, IDS_BAD_COUNT, true);
  expect("n = B + 1", B, {0, 1, 2, 3, 4, 5, 6, 7, 0}, B + 1, IDS_BAD_COUNT);
  expect("n = INT_MAX", B, {0}, 2147483647, IDS_BAD_COUNT);
  expect("NULL list, n = 1", B, {}, 1, IDS_NULL, true);
  expect("one board", B, {3}, 1, IDS_OK);
  expect("first and last", B, {7, 0}, 2, IDS_OK);
  expect("unsorted", B, {5, 1, 6, 2}, 4, IDS_OK);
  expect("n = B", B, {0, 1, 2, 3, 4, 5, 6, 7}, B, IDS_OK);
  expect("n = B, reversed", B, {7, 6, 5, 4, 3, 2, 1, 0}, B, IDS_OK);
  expect("n = B, twice at the end", B, {0, 1, 2, 3, 4, 5, 6, 0}, B, IDS_TWICE);
  expect("twice at the front", B, {4, 4, 1, 2}, 4, IDS_TWICE);
  expect("twice at the back", B, {1, 2, 4, 4}, 4, IDS_TWICE);
  expect("twice, first and last", B, {6, 1, 2, 6}, 4, IDS_TWICE);
  expect("twice, n = 2", B, {0, 0}, 2, IDS_TWICE);
  expect("id -1", B, {-1}, 1, IDS_RANGE);
  expect("id B", B, {B}, 1, IDS_RANGE);
  expect("id -1 at the back", B, {0, 1, -1}, 3, IDS_RANGE);
  expect("id B at the back", B, {0, 1, B}, 3, IDS_RANGE);
  expect("id B at the front", B, {B, 0, 1}, 3, IDS_RANGE);
  expect("id INT_MAX", B, {2, 2147483647}, 2, IDS_RANGE);
  expect("id INT_MIN after good ids", B, {0, 1, -2147483647 - 1}, 3, IDS_RANGE);
  expect("the first fault wins: range", B, {0, 9, 0}, 3, IDS_RANGE);
  expect("the first fault wins: twice", B, {0, 0, 9}, 3, IDS_TWICE);
  // one board, and a scratch vector of another size from the handle before it
  expect("B = 1, n = 1", 1, {0}, 1, IDS_OK);
  expect("B = 1, n = 0", 1, {}, 0, IDS_OK);
  expect("B = 1, id 1", 1, {1}, 1, IDS_RANGE);
  expect("B = 1, n = 2", 1, {0, 0}, 2, IDS_BAD_COUNT);
  expect("B = 70000, far ids", 70000, {69999, 0, 35000}, 3, IDS_OK);
  expect("B = 70000, twice far", 70000, {69999, 1, 69999}, 3, IDS_TWICE);
  if (g_bad) return 1;
  std::printf("ids_check: %d cases ok\n", g_cases);
  return 0;
}
