// td_obs_win.h -- the channel classes of the (45, L, L) observation and the compile-time
// tables of its 1-KB windows (ObsWinTab): a window's channel class, its dirty classes, its
// channels, and the channels a board's written windows read.  Plain C++, no HIP: constants
// and constexpr functions the step kernels read (td_board.h, td_step_obs.h) and
// scripts/channel_needs_host.cpp prints on the host.
#pragma once
#include <stdint.h>

#include "td_common.h"

namespace td {

// Binary observation channels as bits of one word per cell (bit c = channel c):
// 0-3 roads, 4 end, 6-8 starts, 14 buildable (map[6] == 0), 15-16 tower level,
// 17-20 tower type (TDBoard.py:113-133).
constexpr uint32_t kBinaryChannels = 0x1FC1DFu;

// Channel kinds of the observation (TDBoard.get_states, :112-143).
enum ObsKind : int { OK_BIN, OK_CONST, OK_D9, OK_ENEMY };
__host__ __device__ constexpr int obs_kind(int ch) {
  return ch == 9 ? OK_D9
       : (ch < 32 && ((kBinaryChannels >> ch) & 1u)) ? OK_BIN
       : (ch >= 25 && ch < 41) ? OK_ENEMY
       : OK_CONST;
}

// Channel classes of the observation as 64-bit channel masks (TDBoard.get_states,
// :112-143): bits of the packed cell word, the enemy_LP planes, channel 9 (distance
// by table), and the broadcast channels.
constexpr uint64_t kChBin = kBinaryChannels;
constexpr uint64_t kChD9 = 1ull << 9;
constexpr uint64_t kChEnemy = 0xFFFFull << 25;
constexpr uint64_t kChAll = (1ull << NCH) - 1;
constexpr uint64_t kChConst = kChAll & ~(kChBin | kChD9 | kChEnemy);

// Dirty classes of the observation (td_retain_obs): the channels of one class change
// together, and a step that found none of a window's classes dirty leaves the window as
// its last write left it.  STATIC: the layout (roads, end, starts, distance, channel 10),
// new only with a new episode; LP: channel 5 (a leak); TOWER: buildable, tower level / type
// (the tower list changed); COST: channels 21-24 (cost_def crossed a tower cost); ENEMY:
// the enemy planes (the step touched an enemy: U::en_touch, obs_dirty); ALWAYS: costs, progress, channels
// 41-44.
enum : uint32_t { OD_STATIC = 1u, OD_LP = 2u, OD_TOWER = 4u, OD_COST = 8u, OD_ENEMY = 16u, OD_ALWAYS = 32u, OD_ALL = 63u };
__host__ __device__ constexpr uint32_t obs_dirty_class(int ch) {
  return ch == 5 ? OD_LP
       : (ch <= 10) ? OD_STATIC
       : (ch <= 13) ? OD_ALWAYS
       : (ch <= 20) ? OD_TOWER
       : (ch <= 24) ? OD_COST
       : (ch <= 40) ? OD_ENEMY
       : OD_ALWAYS;
}

// The class of every observation window, by the board's misalignment `mis` (units of
// the 128-B line before the board) and window k, as a compile-time table read with one
// scalar load per 8 windows (instead of the window's channel range, channel mask and
// edge test in ~20 SALU per window): bits 0-1 the channel class (0 binary planes only,
// 1 broadcast channels only, 2 enemy planes only, 3 mixed), bit 2 the window holds a
// line shared with a neighbouring board.
// UPL: units per 128-B line, 8 of float32 or 16 of float16 (ObsFmt) -- so many misalignments.
template <int LT, int UPL = 8>
struct ObsWinTab {
  static constexpr int Q = LT * LT / 4, N4 = NCH * Q, K = (N4 + UPL - 1 + 63) / 64, W = (K + 7) / 8;
  struct T { uint32_t w[UPL][W]; };
  // The channels window k overlaps at misalignment mis, bit c = channel c: the window covers
  // the board's units [64 k - mis, 64 k - mis + 63], a channel is Q units.  (A window past the
  // board's last unit, at a small `mis`, has none.)
  static constexpr uint64_t chan(int mis, int k) {
    const int ulo = 64 * k - mis, uhi = ulo + 63;
    const int clo = (ulo < 0 ? 0 : ulo) / Q, chi = (uhi > N4 - 1 ? N4 - 1 : uhi) / Q;
    uint64_t chm = 0;
    for (int c = clo; c <= chi; ++c) chm |= 1ull << c;
    return chm & kChAll;
  }
  static constexpr uint32_t cls(int mis, int k) {
    const int head = mis ? UPL - mis : 0, tail = ((N4 + mis) & ~(UPL - 1)) - mis;
    const int ulo = 64 * k - mis, uhi = ulo + 63;
    const uint64_t chm = chan(mis, k);
    const uint32_t c = (chm & ~kChBin) == 0 ? 0u : (chm & ~kChConst) == 0 ? 1u : (chm & ~kChEnemy) == 0 ? 2u : 3u;
    return c | ((ulo < head || uhi >= tail) ? 4u : 0u);
  }
  static constexpr T make() {
    T t{};
    for (int m = 0; m < UPL; ++m)
      for (int k = 0; k < K; ++k) t.w[m][k / 8] |= cls(m, k) << (4 * (k % 8));
    return t;
  }
  static constexpr T tab = make();
  // The dirty classes (OD_*) whose channels window k overlaps, 8 bits per window: a step
  // that may skip (StepArgs::obs_skip) writes the window only if one of them is dirty.
  static constexpr int WD = (K + 3) / 4;
  struct D { uint32_t w[UPL][WD]; };
  static constexpr uint32_t dirty(int mis, int k) {
    const int ulo = 64 * k - mis, uhi = ulo + 63;
    const int clo = (ulo < 0 ? 0 : ulo) / Q, chi = (uhi > N4 - 1 ? N4 - 1 : uhi) / Q;
    uint32_t d = 0;
    for (int c = clo; c <= chi; ++c) d |= obs_dirty_class(c);
    return d;
  }
  static constexpr D make_d() {
    D t{};
    for (int m = 0; m < UPL; ++m)
      for (int k = 0; k < K; ++k) t.w[m][k / 4] |= dirty(m, k) << (8 * (k % 4));
    return t;
  }
  static constexpr D dtab = make_d();
  // The channels a skipping step's written windows read: a written window is written whole,
  // so it may hold channels of a clean class (window 5 of a 10x10 board holds tower planes
  // beside channel 13; at misalignment 7 window 4 holds the last unit of channel 9).  The
  // set is chan() ORed over the windows one of whose classes is dirty -- done here at compile
  // time for every set a step that kept its episode can have, OD_ALWAYS | any of LP, TOWER,
  // COST, ENEMY (obs_dirty), entry (dirty >> 1) & 15: one scalar load per board.
  static_assert(OD_LP == 2u && OD_TOWER == 4u && OD_COST == 8u && OD_ENEMY == 16u, "ntab's index");
  struct N { uint64_t w[UPL][16]; };
  static constexpr N make_n() {
    N t{};
    for (int m = 0; m < UPL; ++m)
      for (int k = 0; k < K; ++k) {
        const uint32_t d = dirty(m, k);
        const uint64_t c = chan(m, k);
        for (uint32_t i = 0; i < 16; ++i)
          if (d & (OD_ALWAYS | (i << 1))) t.w[m][i] |= c;
      }
    return t;
  }
  static constexpr N ntab = make_n();
};

}  // namespace td
