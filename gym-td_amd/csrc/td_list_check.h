// td_list_check.h -- what the device-side check of a board list (td_step_boards_dev,
// td_copy_boards_dev) shares between the kernel (td_list_check.hip) and the host (td_capi.hip):
// the defect codes (td_list_code, include/tdstep.h), the mark word of the per-board scratch,
// the 64-bit key the defects of one call are combined in, the per-handle record and the
// kernel's arguments.  Plain C++, no HIP: scripts/list_ledger_host.cpp includes it too.
//
// The scratch: one 32-bit word per board, (epoch << 2) | bits.  A call's epoch is its serial
// (list_epoch: 1 .. kListEpochs, then round again), so a word of an earlier call reads as "not
// marked" whatever its bits and the scratch needs no clean-up at all: no O(B) clear, no O(count)
// pass, no kernel boundary (about 1.5-1.9 us) for one.  The host zeroes the scratch on the
// stream once per round of kListEpochs calls (td_capi.hip enqueue_list_check).  A mark is one
// atomic max that returns the old word: kListDst > kListSrc, so a destination's bit stays in
// the word once set, and whichever of two conflicting entries comes second sees the conflict.
#pragma once
#include <stdint.h>

#include "../../include/tdstep.h"

namespace td {

constexpr uint32_t kListSrc = 1u;  // the board is a copy's source
constexpr uint32_t kListDst = 2u;  // the board is a copy's destination, or named by a step's list
constexpr uint32_t kListEpochs = (1u << 30) - 1;
constexpr uint32_t list_epoch(long long call) { return (uint32_t)(call % (long long)kListEpochs) + 1u; }
constexpr uint32_t list_mark(uint32_t epoch, uint32_t bit) { return (epoch << 2) | bit; }
// The bits an entry of `epoch` finds in the old word its mark returned.
constexpr uint32_t list_seen(uint32_t old_word, uint32_t epoch) { return (old_word >> 2) == epoch ? (old_word & 3u) : 0u; }
// What an entry that marks `bit` makes of them: TD_LIST_OK, TD_LIST_TWICE or TD_LIST_OVERLAP.
constexpr int list_conflict(uint32_t seen, uint32_t bit) {
  return bit == kListDst ? ((seen & kListDst) ? TD_LIST_TWICE : (seen & kListSrc) ? TD_LIST_OVERLAP : TD_LIST_OK)
                         : ((seen & kListDst) ? TD_LIST_OVERLAP : TD_LIST_OK);
}

// One defect as a key: a call's verdict is the minimum over its defects, so the lowest code
// wins, and within a code the lowest entry among those detected.  side: 0 the entry of src,
// 1 of dst / boards.  TD_LIST_BAD_COUNT: entry 0 here, -1 in the record (list_verdict).
constexpr unsigned long long kListNoDefect = ~0ull;
constexpr unsigned long long list_key(int code, int entry, int side) {
  return ((unsigned long long)(uint32_t)code << 32) | ((unsigned long long)(uint32_t)entry << 1) | (unsigned)side;
}
constexpr int list_key_code(unsigned long long k) { return k == kListNoDefect ? TD_LIST_OK : (int)(k >> 32); }
constexpr int list_key_entry(unsigned long long k) { return (int)((k & 0xffffffffull) >> 1); }
constexpr int list_key_side(unsigned long long k) { return (int)(k & 1u); }

// The handle's record in device memory (td_create: key = kListNoDefect, the rest zero).
struct ListState {
  unsigned long long key;  // the running check's defects (atomic min); kListNoDefect between calls
  uint32_t arrived;        // blocks of the running check that are through; 0 between calls
  uint32_t refused;        // calls the device refused since the last clear (td_list_errors)
  td_list_status verdict;  // the last check's: what the consumer kernel behind it reads
  td_list_status first;    // the first refused call's since the last clear
};
static_assert(sizeof(td_list_status) == 16 && sizeof(ListState) == 48, "the record's layout");

struct ListCheckArgs {
  const int32_t* src;      // a copy's sources (marked kListSrc), or nullptr: a step's list
  const int32_t* dst;      // a copy's destinations / a step's boards (marked kListDst)
  const int32_t* count;    // [1] entries used, or nullptr: cap
  int cap, B, call;
  uint32_t epoch;          // list_epoch(call)
  uint32_t* marks;         // [B] the scratch
  ListState* st;
  td_list_status* status;  // the caller's copy of the verdict, or nullptr
};

constexpr int kListCheckThreads = 256;  // per block; one thread per entry

}  // namespace td
