// call_check_host.cpp -- what the list calls refuse of a handle's settings and of a device list's
// arguments (gym-td_amd/csrc/td_call_check.h), verdict and whole message, as a host program of its
// own: no HIP, no Python, no GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o call_check_host scripts/call_check_host.cpp && ./call_check_host
//
// Every message buffer is heap memory of exactly the size passed, so a write past it is a
// sanitizer report; an accepted call leaves its buffer untouched.
// Prints "call_check: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <cstring>
#include <string>

#include "../gym-td_amd/csrc/td_call_check.h"

namespace {

int g_cases = 0, g_bad = 0;
const size_t kCap = 240;

void verdict(const char* what, bool ok, const char* msg) {
  ++g_cases;
  if (!ok && !g_bad++) std::printf("FAIL %s: msg '%s'\n", what, msg);
}

void expect_partial(const char* fn, int frame_skip, int opp_np, int autoreset, const std::string& want) {
  char* msg = new char[kCap];
  std::memset(msg, '#', kCap);
  msg[kCap - 1] = 0;
  const bool refused = td::partial_step_refused(fn, frame_skip, opp_np, autoreset, msg, kCap);
  verdict(fn, refused == !want.empty() && (refused ? want == msg : msg[0] == '#'), msg);
  delete[] msg;
}

void expect_list(const char* fn, int cap, int B, bool have, const char* lists, int want_rc, const std::string& want) {
  char* msg = new char[kCap];
  std::memset(msg, '#', kCap);
  msg[kCap - 1] = 0;
  const int rc = td::list_args_check(fn, cap, B, have, lists, msg, kCap);
  verdict(fn, rc == want_rc && (rc == td::LIST_ARGS_REFUSED ? want == msg : msg[0] == '#'), msg);
  delete[] msg;
}

}  // namespace

int main() {
  using namespace td;
  const std::string tail_skip = "); set td_set_frame_skip(h, 1) first";
  const std::string np = ": not supported with random_agent = 0 and auto-reset on (the reset kernel behind a step goes by "
                         "done[] of every board, and an unnamed board's is stale)";
  for (const char* fn : {"td_step_boards", "td_step_boards_dev"}) {
    const std::string f = fn;
    // accepted: no frame skip, and random_agent = 0 or auto-reset but not both
    for (int opp_np = 0; opp_np < 2; ++opp_np)
      for (int autoreset = 0; autoreset < 2; ++autoreset)
        if (!(opp_np && autoreset)) expect_partial(fn, 1, opp_np, autoreset, "");
    expect_partial(fn, 1, 1, 1, f + np);
    // frame skip, with its k in the message; it wins over random_agent = 0
    for (int k : {2, 16})
      for (int both = 0; both < 2; ++both)
        expect_partial(fn, k, both, both, f + ": not supported with frame skip (td_frame_skip() = " + std::to_string(k) + tail_skip);
  }
  const int B = 4;
  for (const char* fn : {"td_step_boards_dev", "td_copy_boards_dev", "td_action_mask_boards_dev"}) {
    const std::string f = fn;
    const char* lists = fn[3] == 'c' ? "src_dev or dst_dev" : "boards_dev";
    // cap < 0 whatever B is (B = 0: the test in front of the handle) and whatever the pointers are
    for (int b : {0, B})
      for (int have = 0; have < 2; ++have) {
        expect_list(fn, -1, b, have, lists, LIST_ARGS_REFUSED, f + ": cap = -1 is negative");
        expect_list(fn, -2147483647 - 1, b, have, lists, LIST_ARGS_REFUSED, f + ": cap = -2147483648 is negative");
      }
    // cap > B wins over a NULL list
    for (int have = 0; have < 2; ++have) {
      expect_list(fn, B + 1, B, have, lists, LIST_ARGS_REFUSED, f + ": cap = 5 outside [0, 4] (the handle's boards)");
      expect_list(fn, 2147483647, B, have, lists, LIST_ARGS_REFUSED,
                  f + ": cap = 2147483647 outside [0, 4] (the handle's boards)");
      expect_list(fn, 0, B, have, lists, LIST_ARGS_EMPTY, "");  // an empty list, NULL or not
    }
    for (int cap : {1, B}) {
      expect_list(fn, cap, B, true, lists, LIST_ARGS_GO, "");
      expect_list(fn, cap, B, false, lists, LIST_ARGS_REFUSED, f + ": " + lists + " is NULL with cap = " + std::to_string(cap));
    }
    expect_list(fn, 1, 1, true, lists, LIST_ARGS_GO, "");  // one board
    expect_list(fn, 2, 1, true, lists, LIST_ARGS_REFUSED, f + ": cap = 2 outside [0, 1] (the handle's boards)");
  }
  if (g_bad) return 1;
  std::printf("call_check: %d cases ok\n", g_cases);
  return 0;
}
