// td_obs_ledger.h -- what a handle knows of its retained observation buffer (td_retain_obs,
// include/tdstep.h): the pointer, and which boards' observations it holds as this handle's
// last write left them.  Plain C++, no HIP: td_capi.hip's entry points call it around their
// launches, and scripts/obs_ledger_host.cpp runs the header's contract alone, case by case.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace td {

struct ObsLedger {
  int B = 0;  // the handle's boards (td_create)
  // the buffer the caller leaves to this handle's own writes, and whether it holds every
  // board's observation as this handle's last write left it (touch clears it)
  const void* retained = nullptr;
  bool retained_valid = false;     // every board's is known to be there
  std::vector<uint8_t> obs_known;  // [B] board b's is (a reset into the buffer wrote it, or a step)
  int n_known = 0;

  // Some board's observation would now differ from what the retained buffer holds, and
  // nothing wrote it there: the next step writes every byte (td_retain_obs).
  void touch() {
    retained_valid = false;
    if (n_known) std::fill(obs_known.begin(), obs_known.end(), (uint8_t)0);
    n_known = 0;
  }
  // Board b's observation was just written whole into the retained buffer.
  void mark(int b) {
    if (obs_known.size() != (size_t)B) obs_known.assign((size_t)B, 0);
    if (!obs_known[(size_t)b]) {
      obs_known[(size_t)b] = 1;
      n_known += 1;
    }
    retained_valid = n_known == B;
  }
  // Every board's was (a step into the retained buffer).
  void mark_all() {
    obs_known.assign((size_t)B, 1);
    n_known = B;
    retained_valid = true;
  }
  // Whether `obs` is the retained buffer.
  bool is_retained(const void* obs) const { return retained && obs == retained; }
  // A reset that writes into `obs`: the boards it resets are written whole.  Into the
  // retained buffer that keeps it current; anywhere else (or nowhere) leaves it behind.
  bool reset_into(const void* obs) {
    const bool mine = is_retained(obs);
    if (!mine) touch();
    return mine;
  }
  // A step of every board into `obs` may skip what the buffer already holds.
  bool full_step_skips(const void* obs) const { return is_retained(obs) && retained_valid; }
  // A step of boards[0 .. n) (checked ids) into `obs` may: every one of them is known.
  bool partial_step_skips(const void* obs, const int32_t* boards, int n) const {
    bool known = is_retained(obs) && (retained_valid || obs_known.size() == (size_t)B);
    for (int i = 0; known && !retained_valid && i < n; ++i) known = obs_known[(size_t)boards[i]] != 0;
    return known;
  }
  // Device-resident lists (td_step_boards_dev, td_copy_boards_dev): the host does not know
  // which boards a call names, nor whether the device will accept the list, so these never
  // mark a board: no sequence of them raises n_known or sets retained_valid.
  // A step of a device list into `obs` may skip only if every board is known.
  bool list_step_skips(const void* obs) const { return full_step_skips(obs); }
  // After such a step, or a device-list copy, into `obs` (nullptr: a copy without rows).  Into
  // the retained buffer the set of known boards stays as it was: a known board's row was
  // written whole or in its dirty windows, an unknown one's whole, but which cannot be marked;
  // a refused list changed nothing.  Any other buffer leaves the retained one behind, as the
  // host-list forms do.  Whether `obs` is the retained buffer.
  bool list_call_into(const void* obs) {
    const bool mine = is_retained(obs);
    if (!mine) touch();
    return mine;
  }
  // The block [p, p + bytes) was freed (a record of no size counts as one byte): a later
  // allocation may reuse the address, which must not be taken for the retained buffer.
  // Whether the retention was dropped.
  bool freed(const void* p, size_t bytes) {
    const char* lo = static_cast<const char*>(p);
    const char* r = static_cast<const char*>(retained);
    if (!(r && r >= lo && r < lo + std::max<size_t>(bytes, 1))) return false;
    retained = nullptr;
    touch();
    return true;
  }
  // A call that returns early with an error leaves the retained buffer behind.
  struct Guard {
    ObsLedger* l;
    bool ok = false;
    ~Guard() {
      if (!ok) l->touch();
    }
  };
};

}  // namespace td
