// td_mask_body.h -- the mask of one board, by one wave: the common body of td_mask_kernel
// (td_mask.hip, every board) and td_mask_list_kernel (td_mask_list.hip, the boards of a list),
// and in front of it the row build, which the sampler (td_sample.hip) runs too.
// Device text only; each kernel supplies the wave's LDS row.
//
// The wave reads the board's header (96 B), its cell words (map[6], the build-blocking count,
// in bits 24-31) and its tower words, puts the board's row together in LDS -- one byte per
// action, op-major like the action index a = op * L^2 + cell -- and stores it.  The verdicts
// are td_mask.h's: the step's own comparisons on the same f64 / integer values, so the mask is
// exact.
//
// (The tower on a cell is not in the HBM cell word -- store_cells masks the tower nibble,
// which lives only in the step's LDS copy -- so level-up and destruct read the tower list:
// every cell starts as "no tower there", then the board's <= 32 tower lanes overwrite the
// two entries of their own cells.)
//
// Stores: the row lies in LDS at the same offset mod 16 as in global memory, so every 16-B
// piece of global memory that the row covers whole is one aligned ds_read_b128 and one
// global_store_dwordx4; the pieces a row shares with its neighbours (its first and last,
// unless row start and pitch are multiples of 16) go out byte by byte.  Same bytes either
// way, and nothing outside [b * pitch, (b + 1) * pitch) is written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "td_kernels.h"
#include "td_list_dev.h"
#include "td_mask.h"
#include "td_step_launch.h"
#include "td_wave.h"

namespace td {

namespace {

// LDS bytes of a row: the alignment shift (< 16), 6 L^2 + 1 actions, rounded up to 16
template <int LT>
struct MaskRow {
  static constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  static constexpr int BYTES = (15 + 6 * NC + 1 + 15) & ~15;
};

// `n` bytes of the row from LDS offset `off` (byte `off` of the 16-B grid = global address
// g - (g & 15)): row bytes past the LDS image are padding inside the pitch.
template <int RB>
__device__ __forceinline__ uint32_t row_byte(const uint8_t* R, int j) { return j < RB ? R[j] : kMaskPad; }

// ---- the row build: the legality rules' one device restatement, shared with the sampler
// (td_sample.hip).  What differs between the two stays in their bodies: the padding fill, the
// mask's alignment shift and no-op byte, where the wave syncs, the sampler's early exit.

// The board's header: 24 words, one per lane, and the values as lane broadcasts of them (TdHdr,
// td_common.h), each evaluated where it is asked for.
struct HdrWords {
  static_assert(offsetof(TdHdr, cost_def) == 0 && offsetof(TdHdr, cost_atk) == 8 && offsetof(TdHdr, steps) == 24 &&
                offsetof(TdHdr, atk_cd) == 32 && offsetof(TdHdr, def_cd) == 36 && offsetof(TdHdr, n_en) == 40 &&
                offsetof(TdHdr, n_tw) == 44 && offsetof(TdHdr, num_roads) == 48, "TdHdr words read below");
  uint32_t w;
  __device__ __forceinline__ HdrWords(const TdHdr* hdr, int lane)
      : w(lane < (int)(sizeof(TdHdr) / 4) ? reinterpret_cast<const uint32_t*>(hdr)[lane] : 0u) {}
  __device__ __forceinline__ int word(int i) const { return (int)rdl(w, i); }
  __device__ __forceinline__ double cost_def() const { return __hiloint2double(word(1), word(0)); }
  __device__ __forceinline__ double cost_atk() const { return __hiloint2double(word(3), word(2)); }
  __device__ __forceinline__ int steps() const { return word(6); }
  __device__ __forceinline__ int atk_cd() const { return word(8); }
  __device__ __forceinline__ int def_cd() const { return word(9); }
  __device__ __forceinline__ int n_en() const { return word(10); }
  __device__ __forceinline__ int n_tw() const { return word(11); }
  __device__ __forceinline__ int num_roads() const { return word(12); }
};

// Build (ops 0-3) per cell of board b into ROW[op * NC + cell]; level-up / destruct (ops 4-5):
// no tower there.  Then, behind the caller's wsync(), the board's n_tw <= TCAP tower lanes
// overwrite the two entries of their own cells.  Macros, not functions, as td_copy_body.h's
// body and for its reason: a function boundary around the cell pass changes how the compiler
// forms the branch on NC & 3 in the generic-side kernels (two instructions, measured with
// scripts/kernel_isa_digest.py); as macros every kernel's token stream is what it was.  In
// scope at the expansion: v (the BoardView), C (*v.cfg), b, NC, lane, cost_def, n_tw.
#define TD_ROW_CELLS(ROW)                                                                                        \
  double price[4];                                                                                               \
  _Pragma("unroll") for (int t = 0; t < 4; ++t) price[t] = C.t_price[t][0];                                      \
  const uint32_t* const cw = v.cells + (size_t)b * NC;                                                           \
  auto put_cell = [&](int c, uint32_t word) {                                                                    \
    _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                \
        (ROW)[t * NC + c] = (uint8_t)mask_build_code(cost_def, price[t], word, n_tw);                            \
    (ROW)[4 * NC + c] = (uint8_t)mask_lvup_code(false, 0u, cost_def, C);                                         \
    (ROW)[5 * NC + c] = (uint8_t)mask_destruct_code(false);                                                      \
  };                                                                                                             \
  if ((NC & 3) == 0) { /* 16-B loads of four cells (the board's words start 16-B aligned) */                     \
    const u32x4* const cw4 = reinterpret_cast<const u32x4*>(cw);                                                 \
    for (int i = lane; i < NC / 4; i += 64) {                                                                    \
      const u32x4 x = cw4[i];                                                                                    \
      put_cell(4 * i + 0, x.x); put_cell(4 * i + 1, x.y); put_cell(4 * i + 2, x.z); put_cell(4 * i + 3, x.w);    \
    }                                                                                                            \
  } else {                                                                                                       \
    for (int c = lane; c < NC; c += 64) put_cell(c, cw[c]);                                                      \
  }
#define TD_ROW_TOWERS(ROW)                                                                                       \
  if (lane < n_tw) { /* (one tower per cell: no two lanes write the same byte) */                                \
    const uint32_t ti = v.tw_inf[(size_t)b * TCAP + lane];                                                       \
    const int c = tw_cell(ti);                                                                                   \
    if (c < NC) {                                                                                                \
      (ROW)[4 * NC + c] = (uint8_t)mask_lvup_code(true, ti, cost_def, C);                                        \
      (ROW)[5 * NC + c] = (uint8_t)mask_destruct_code(true);                                                     \
    }                                                                                                            \
  }

// R: the wave's own MaskRow<LT>::BYTES of LDS, 16-B aligned; only wsync() orders its accesses.
template <int LT>
__device__ __forceinline__ void mask_board(const MaskArgs& a, int b, int lane, uint8_t* const R) {
  constexpr int RB = MaskRow<LT>::BYTES;
  const BoardView& v = a.v;
  const int L = LT ? LT : v.L, NC = L * L;
  const TdDevCfg& C = *v.cfg;

  const HdrWords hd(v.hdr + b, lane);
  const double cost_def = hd.cost_def();
  const double cost_atk = hd.cost_atk();
  const int steps = hd.steps(), atk_cd = hd.atk_cd(), def_cd = hd.def_cd();
  const int n_en = hd.n_en(), num_roads = hd.num_roads();
  int n_tw = hd.n_tw();
  const bool live = mask_board_live(num_roads);

  if (a.atk_mask && lane < 15) {  // [3][5]: road, type (4 = none: always legal)
    const int road = lane / 5, t = lane - 5 * road;
    const bool ok = t == 4 || mask_summon_ok(road, t & 3, mask_enemy_lv(steps, C), num_roads, atk_cd, n_en, cost_atk, C);
    a.atk_mask[(size_t)b * 15 + lane] = ok ? 1 : 0;
  }
  if (!a.def_mask && !a.def_code) return;

  const size_t pitch = a.def_pitch;
  const size_t g = (size_t)b * pitch;  // the row's first byte (the same in def_mask and def_code)
  // LDS image: byte i of the row at R[sh + i], sh = the row's global address mod 16 (both
  // outputs must agree on it for the 16-B path; else the per-byte path below)
  const uintptr_t pm = reinterpret_cast<uintptr_t>(a.def_mask), pc = reinterpret_cast<uintptr_t>(a.def_code);
  const uintptr_t p0 = a.def_mask ? pm : pc;
  const int sh = (int)((p0 + g) & 15u);
  const bool same_phase = !a.def_mask || !a.def_code || ((pm ^ pc) & 15u) == 0;

  {  // padding everywhere first (16-B LDS stores)
    const u32x4 pad = {kMaskPad * 0x01010101u, kMaskPad * 0x01010101u, kMaskPad * 0x01010101u, kMaskPad * 0x01010101u};
    u32x4* R4 = reinterpret_cast<u32x4*>(R);
    for (int i = lane; i < RB / 16; i += 64) R4[i] = pad;
  }
  wsync();
  if (n_tw > TCAP) n_tw = TCAP;  // (never by the step's own stores: an imported header)
  uint8_t* const row = R + sh;
  TD_ROW_CELLS(row)
  if (lane == 0 && !v.multi) row[6 * NC] = (uint8_t)kMaskAlways;  // the no-op
  wsync();
  TD_ROW_TOWERS(row)
  wsync();

  // out: bytes [sh, sh + pitch) of the 16-B grid that starts at global address p0 + g - sh
  const bool open = live && mask_cd_open(def_cd);
  const int end = sh + (int)pitch;  // (pitch <= kMaskMaxPitch)
  uint8_t* const gm = a.def_mask ? a.def_mask + g - sh : nullptr;
  uint8_t* const gc = a.def_code ? a.def_code + g - sh : nullptr;
  auto put_bytes = [&](int j0, int j1) {  // grid bytes [j0, j1) one by one
    for (int j = j0 + lane; j < j1; j += 64) {
      const uint32_t x = row_byte<RB>(R, j);
      if (gm) gm[j] = (uint8_t)(mask_legal4(x, open) & 1u);
      if (gc) gc[j] = (uint8_t)(mask_code4(x) & 0xffu);
    }
  };
  if (!same_phase) {
    put_bytes(sh, end);
    return;
  }
  const int k0 = (sh + 15) >> 4, k1 = end >> 4;  // whole 16-B pieces [k0, k1)
  if (k0 >= k1) {
    put_bytes(sh, end);
    return;
  }
  put_bytes(sh, 16 * k0);
  const u32x4* const R4 = reinterpret_cast<const u32x4*>(R);
  for (int k = k0 + lane; k < k1; k += 64) {
    u32x4 x = {kMaskPad * 0x01010101u, kMaskPad * 0x01010101u, kMaskPad * 0x01010101u, kMaskPad * 0x01010101u};
    if (16 * k + 16 <= RB) x = R4[k];
    if (gm) {
      const u32x4 m = {mask_legal4(x.x, open), mask_legal4(x.y, open), mask_legal4(x.z, open), mask_legal4(x.w, open)};
      *reinterpret_cast<u32x4*>(gm + 16 * (size_t)k) = m;
    }
    if (gc) {
      const u32x4 c = {mask_code4(x.x), mask_code4(x.y), mask_code4(x.z), mask_code4(x.w)};
      *reinterpret_cast<u32x4*>(gc + 16 * (size_t)k) = c;
    }
  }
  put_bytes(16 * k1, end);
}

}  // namespace

}  // namespace td
