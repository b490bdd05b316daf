// td_mask_body.h -- the mask of one board, by one wave: the common body of td_mask_kernel
// (td_mask.hip, every board) and td_mask_list_kernel (td_mask_list.hip, the boards of a list).
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
#include "td_mask.h"
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

// R: the wave's own MaskRow<LT>::BYTES of LDS, 16-B aligned; only wsync() orders its accesses.
template <int LT>
__device__ __forceinline__ void mask_board(const MaskArgs& a, int b, int lane, uint8_t* const R) {
  constexpr int RB = MaskRow<LT>::BYTES;
  const int L = LT ? LT : a.L, NC = L * L;
  const TdDevCfg& C = *a.cfg;

  // the header: 24 words, one per lane, then lane broadcasts (TdHdr, td_common.h)
  const uint32_t* const hw = reinterpret_cast<const uint32_t*>(a.hdr + b);
  const uint32_t w = lane < (int)(sizeof(TdHdr) / 4) ? hw[lane] : 0u;
  static_assert(offsetof(TdHdr, cost_def) == 0 && offsetof(TdHdr, cost_atk) == 8 && offsetof(TdHdr, steps) == 24 &&
                offsetof(TdHdr, atk_cd) == 32 && offsetof(TdHdr, def_cd) == 36 && offsetof(TdHdr, n_en) == 40 &&
                offsetof(TdHdr, n_tw) == 44 && offsetof(TdHdr, num_roads) == 48, "TdHdr words read below");
  const double cost_def = __hiloint2double((int)rdl(w, 1), (int)rdl(w, 0));
  const double cost_atk = __hiloint2double((int)rdl(w, 3), (int)rdl(w, 2));
  const int steps = (int)rdl(w, 6), atk_cd = (int)rdl(w, 8), def_cd = (int)rdl(w, 9);
  const int n_en = (int)rdl(w, 10), num_roads = (int)rdl(w, 12);
  int n_tw = (int)rdl(w, 11);
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
  // build (ops 0-3) per cell; level-up / destruct (ops 4-5): no tower there
  if (n_tw > TCAP) n_tw = TCAP;  // (never by the step's own stores: an imported header)
  double price[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) price[t] = C.t_price[t][0];
  uint8_t* const row = R + sh;
  const uint32_t* const cw = a.cells + (size_t)b * NC;
  auto put_cell = [&](int c, uint32_t word) {
#pragma unroll
    for (int t = 0; t < 4; ++t) row[t * NC + c] = (uint8_t)mask_build_code(cost_def, price[t], word, n_tw);
    row[4 * NC + c] = (uint8_t)mask_lvup_code(false, 0u, cost_def, C);
    row[5 * NC + c] = (uint8_t)mask_destruct_code(false);
  };
  if ((NC & 3) == 0) {  // 16-B loads of four cells (the board's words start 16-B aligned)
    const u32x4* const cw4 = reinterpret_cast<const u32x4*>(cw);
    for (int i = lane; i < NC / 4; i += 64) {
      const u32x4 v = cw4[i];
      put_cell(4 * i + 0, v.x); put_cell(4 * i + 1, v.y); put_cell(4 * i + 2, v.z); put_cell(4 * i + 3, v.w);
    }
  } else {
    for (int c = lane; c < NC; c += 64) put_cell(c, cw[c]);
  }
  if (lane == 0 && !a.multi) row[6 * NC] = (uint8_t)kMaskAlways;  // the no-op
  wsync();
  if (lane < n_tw) {  // (one tower per cell: no two lanes write the same byte)
    const uint32_t ti = a.tw_inf[(size_t)b * TCAP + lane];
    const int c = tw_cell(ti);
    if (c < NC) {
      row[4 * NC + c] = (uint8_t)mask_lvup_code(true, ti, cost_def, C);
      row[5 * NC + c] = (uint8_t)mask_destruct_code(true);
    }
  }
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
