// playout_check_host.cpp -- what td_playout and its list forms refuse of their io and of the
// handle's settings (gym-td_amd/csrc/td_call_check.h playout_io_refused), verdict and whole
// message, as a host program of its own: no HIP, no Python, no GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o playout_check_host scripts/playout_check_host.cpp && ./playout_check_host
//
// Every message buffer is heap memory of exactly the size passed, so a write past it is a
// sanitizer report; an accepted call leaves its buffer untouched.  The refusals are tried one
// by one and then in pairs: of two faults the one earlier in the order wins.
// Prints "playout_check: N cases ok" and returns 0, or names the first case that went wrong.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../gym-td_amd/csrc/td_call_check.h"

namespace {

int g_cases = 0, g_bad = 0;
const size_t kCap = 240;
const unsigned kSize = 120;
const int kAbi = 3, kMax = 4096;

void expect(const char* fn, const td::PlayoutIoSeen& v, const std::string& want) {
  char* msg = new char[kCap];
  std::memset(msg, '#', kCap);
  msg[kCap - 1] = 0;
  const bool refused = td::playout_io_refused(fn, v, kSize, kAbi, kMax, msg, kCap);
  ++g_cases;
  const bool ok = refused == !want.empty() && (refused ? want == msg : msg[0] == '#');
  if (!ok && !g_bad++) std::printf("FAIL %s: want '%s', msg '%s'\n", fn, want.c_str(), msg);
  delete[] msg;
}

td::PlayoutIoSeen good(int mode) {
  td::PlayoutIoSeen v;
  v.io = true; v.size = kSize; v.abi = (unsigned)kAbi; v.handle = true;
  v.steps = 5; v.reward = v.done = true; v.mode = mode;
  return v;
}

// The faults in refusal order: how to plant one, and the message's tail behind the call's name.
struct Fault {
  void (*plant)(td::PlayoutIoSeen&);
  const char* tail;
};

}  // namespace

int main() {
  using namespace td;
  const std::vector<Fault> faults = {
      {[](PlayoutIoSeen& v) { v.io = false; }, ": NULL io"},
      {[](PlayoutIoSeen& v) { v.size = 112; },
       ": td_playout_io has size 112 / abi 3, this library expects size 120 / abi 3 (call td_playout_io_init)"},
      {[](PlayoutIoSeen& v) { v.handle = false; }, ": NULL handle"},
      {[](PlayoutIoSeen& v) { v.steps = 0; }, ": steps = 0 outside [1, 4096] (TD_MAX_PLAYOUT_STEPS)"},
      {[](PlayoutIoSeen& v) { v.done = false; }, ": reward and done are required"},
      {[](PlayoutIoSeen& v) { v.mode = 1; v.first_def = true; }, ": TD-atk has no defender side (first_def)"},
      {[](PlayoutIoSeen& v) { v.multi = 1; },
       ": not supported with multi-action (the playout samples one discrete action per side and sub-step)"},
      {[](PlayoutIoSeen& v) { v.opp_np = 1; },
       ": not supported with random_agent = 0 (the built-in opponent would draw from the layout stream inside the "
       "launch)"},
  };
  for (const char* fn : {"td_playout", "td_playout_boards", "td_playout_boards_dev"}) {
    const std::string f = fn;
    // accepted: every mode, both ends of steps, the first actions of the sides the mode has
    for (int mode = 0; mode < 3; ++mode) {
      PlayoutIoSeen v = good(mode);
      expect(fn, v, "");
      v.steps = 1; expect(fn, v, "");
      v.steps = kMax; expect(fn, v, "");
      v.first_def = mode != 1; v.first_atk = mode != 0;
      expect(fn, v, "");
    }
    // one fault each, then two: the earlier one's message
    for (size_t i = 0; i < faults.size(); ++i) {
      PlayoutIoSeen v = good(0);
      faults[i].plant(v);
      expect(fn, v, f + faults[i].tail);
      for (size_t j = i + 1; j < faults.size(); ++j) {
        PlayoutIoSeen w = good(0);
        faults[j].plant(w);  // (the later one first: planting mode = 1 must not undo the earlier)
        faults[i].plant(w);
        expect(fn, w, f + faults[i].tail);
      }
    }
    // the variants of each fault
    PlayoutIoSeen v = good(0);
    v.abi = 2;
    expect(fn, v, f + ": td_playout_io has size 120 / abi 2, this library expects size 120 / abi 3 (call td_playout_io_init)");
    for (int steps : {-1, kMax + 1, -2147483647 - 1, 2147483647}) {
      v = good(2);
      v.steps = steps;
      expect(fn, v, f + ": steps = " + std::to_string(steps) + " outside [1, 4096] (TD_MAX_PLAYOUT_STEPS)");
    }
    v = good(2); v.reward = false;
    expect(fn, v, f + ": reward and done are required");
    v = good(0); v.first_atk = true;
    expect(fn, v, f + ": TD-def has no attacker side (first_atk)");
    v = good(1); v.first_atk = true;
    expect(fn, v, "");
    v = good(2); v.first_def = v.first_atk = true; v.multi = 1; v.opp_np = 1;
    expect(fn, v, f + faults[6].tail);
  }
  if (g_bad) return 1;
  std::printf("playout_check: %d cases ok\n", g_cases);
  return 0;
}
