// td_state_rec.h -- the record td_export_state writes and td_import_state reads: for `count`
// boards, eight arrays one behind the other, each board-major (all headers, then all en_lp, ...).
// Plain C++, no HIP: one table gives the sizes and offsets, and what an import does to a record
// before it is uploaded are functions of a host buffer.  td_capi.hip keeps the copies;
// scripts/state_rec_host.cpp runs this header alone under the address and undefined-behaviour
// sanitizers.  The Python mirror of the table is gym_TD.engine._layout.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstdio>

#include "td_common.h"
#include "td_layout.h"  // MAX_ROAD_CELLS (and td_rng.h: MT_N)

namespace td {

// The record's arrays in record order: bytes per board, fixed + per_cell * L^2.
struct StateRecArray {
  const char* name;
  size_t fixed, per_cell;
};
enum : int { SR_HDR, SR_EN_LP, SR_EN_MG, SR_EN_INF, SR_TW_CD, SR_TW_INF, SR_CELLS, SR_OPP_MT, SR_ARRAYS };
constexpr StateRecArray kStateRec[SR_ARRAYS] = {
    {"hdr", sizeof(TdHdr), 0},
    {"en_lp", sizeof(double) * ECAP, 0},
    {"en_mg", sizeof(double) * ECAP, 0},
    {"en_inf", sizeof(uint32_t) * ECAP, 0},
    {"tw_cd", sizeof(double) * TCAP, 0},
    {"tw_inf", sizeof(uint32_t) * TCAP, 0},
    {"cells", 0, sizeof(uint32_t)},
    {"opp_mt", sizeof(uint32_t) * OPP_WORDS, 0}};

constexpr size_t state_rec_elem(int k, int NC) { return kStateRec[k].fixed + kStateRec[k].per_cell * (size_t)NC; }
// Byte offset of array k in a record of `count` boards; k = SR_ARRAYS: the record's size.
constexpr size_t state_rec_offset(int k, int NC, size_t count) {
  size_t per_board = 0;
  for (int j = 0; j < k; ++j) per_board += state_rec_elem(j, NC);
  return count * per_board;
}
constexpr size_t state_rec_bytes(int NC, size_t count) { return state_rec_offset(SR_ARRAYS, NC, count); }
static_assert(state_rec_bytes(100, 1) == 5944, "the record at L = 10");

// td_import_state's header checks, board by board: 0, or -1 with the first fault in msg.
// A record whose board has a layout must carry the captured max_cost / max_base_LP the
// step divides by (TdHdr.format: header format 2); a record of another format, or a
// hand-built one with zeros there, would silently clamp every cost to 0 and divide the
// observation's scalar channels by zero.  b0: the first board's id, for the message.
inline int state_rec_check(const TdHdr* hdr, int count, int b0, char* msg, size_t cap) {
  for (int i = 0; i < count; ++i) {
    const TdHdr& x = hdr[i];
    if (x.num_roads < 1 || x.num_roads > 3) continue;  // a board never reset: nothing is stepped
    if (x.format != kHdrFormat) {
      std::snprintf(msg, cap, "board %d: header format 0x%x, expected 0x%x (a record of another build?)", b0 + i,
                    (unsigned)x.format, (unsigned)kHdrFormat);
      return -1;
    }
    if (!(x.max_cost > 0.0) || x.max_base_LP < 1) {
      std::snprintf(msg, cap, "board %d: max_cost %g / max_base_LP %d (must be > 0 / >= 1)", b0 + i, x.max_cost,
                    x.max_base_LP);
      return -1;
    }
    if (x.n_en < 0 || x.n_en > ECAP || x.n_tw < 0 || x.n_tw > TCAP) {
      std::snprintf(msg, cap, "board %d: %d enemies / %d towers exceed the capacity", b0 + i, x.n_en, x.n_tw);
      return -1;
    }
    if (x.maxdist < 0 || x.maxdist > MAX_ROAD_CELLS - 1) {
      std::snprintf(msg, cap, "board %d: max dist %d (must be 0..%d: a road has at most %d cells)", b0 + i, x.maxdist,
                    MAX_ROAD_CELLS - 1, MAX_ROAD_CELLS);
      return -1;
    }
  }
  return 0;
}

// An imported record (the caller's copy of it) takes the importing engine's config epoch:
// imported enemies and towers take the current one, since epoch tags of another engine (or
// of blocks since recycled) mean nothing here.  Cell words: bits 10-15 are not part of the
// layout format (the step keeps the tower of a cell there in LDS only).
inline void state_rec_retag(uint8_t* rec, int NC, size_t count, int epoch) {
  uint32_t* einf = (uint32_t*)(rec + state_rec_offset(SR_EN_INF, NC, count));
  uint32_t* tinf = (uint32_t*)(rec + state_rec_offset(SR_TW_INF, NC, count));
  uint32_t* cw = (uint32_t*)(rec + state_rec_offset(SR_CELLS, NC, count));
  for (size_t i = 0; i < count * ECAP; ++i) einf[i] = (einf[i] & 0x00ffffffu) | ((uint32_t)epoch << 24);
  for (size_t i = 0; i < count * TCAP; ++i)
    tinf[i] = (tinf[i] & 0x0000ffffu) | ((uint32_t)epoch << 16) | ((uint32_t)epoch << 24);
  for (size_t i = 0; i < count * (size_t)NC; ++i) cw[i] &= ~(0x3Fu << 10);
}

// The opponent stream's position and lazy boundary, opp_mt[MT_N] and [MT_N + 1] in a record,
// live in the first two words of the board's hot record on the device (hot_stride words per
// board).  An import sets them there (no pre-drawn outputs: the caller zeroes the rest), an
// export takes them from there.
inline void state_rec_pos_to_hot(const uint32_t* opp, uint32_t* hot, size_t hot_stride, size_t count) {
  for (size_t i = 0; i < count; ++i) {
    hot[i * hot_stride] = opp[i * OPP_WORDS + MT_N];
    hot[i * hot_stride + 1] = opp[i * OPP_WORDS + MT_N + 1];
  }
}
inline void state_rec_pos_from_hot(uint32_t* opp, const uint32_t* hot, size_t hot_stride, size_t count) {
  for (size_t i = 0; i < count; ++i) {
    opp[i * OPP_WORDS + MT_N] = hot[i * hot_stride];
    opp[i * OPP_WORDS + MT_N + 1] = hot[i * hot_stride + 1];
  }
}

}  // namespace td
