// channel_needs_host.cpp -- the observation's window tables (gym-td_amd/csrc/td_obs_win.h
// ObsWinTab) printed as text, as a host program of its own: no HIP, no Python, no GPU.
// tests/test_channel_needs_host.py compares the lines with a plain restatement of the windows.
//
//   c++ -std=c++17 -o channel_needs_host scripts/channel_needs_host.cpp && ./channel_needs_host
//
// One line per entry, for L = 10, 20, 30 and 8 / 16 units per 128-B line:
//   chan  L UPL mis k <channel mask, hex>      the channels window k overlaps
//   dirty L UPL mis k <dirty classes, hex>     ... and their dirty classes (as stored in dtab)
//   need  L UPL mis i <channel mask, hex>      the channels the written windows read when
//                                              the dirty classes are OD_ALWAYS | i << 1
#include <cstdio>

#define __host__
#define __device__
#include "../gym-td_amd/csrc/td_obs_win.h"

namespace {

template <int LT, int UPL>
void dump() {
  typedef td::ObsWinTab<LT, UPL> Tab;
  static_assert(Tab::tab.w[0][0] == (Tab::cls(0, 0) | Tab::cls(0, 1) << 4 | Tab::cls(0, 2) << 8 | Tab::cls(0, 3) << 12 |
                                     Tab::cls(0, 4) << 16 | Tab::cls(0, 5) << 20 | Tab::cls(0, 6) << 24 | Tab::cls(0, 7) << 28),
                "class table packing");
  std::printf("shape %d %d K %d\n", LT, UPL, Tab::K);
  for (int m = 0; m < UPL; ++m) {
    for (int k = 0; k < Tab::K; ++k) {
      std::printf("chan %d %d %d %d %llx\n", LT, UPL, m, k, (unsigned long long)Tab::chan(m, k));
      std::printf("dirty %d %d %d %d %x\n", LT, UPL, m, k, (Tab::dtab.w[m][k / 4] >> (8 * (k % 4))) & 0xffu);
    }
    for (int i = 0; i < 16; ++i) std::printf("need %d %d %d %d %llx\n", LT, UPL, m, i, (unsigned long long)Tab::ntab.w[m][i]);
  }
}

}  // namespace

int main() {
  dump<10, 8>();
  dump<10, 16>();
  dump<20, 8>();
  dump<20, 16>();
  dump<30, 8>();
  dump<30, 16>();
  return 0;
}
