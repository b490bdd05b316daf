// td_call_check.h -- what the list calls refuse of the handle's settings and of a device list's
// arguments, each written once.  Plain C++, no HIP: functions of the handle's ints that write a
// message and take the caller's name; td_capi.hip calls them before anything is enqueued, and
// scripts/call_check_host.cpp runs them alone.  (The contents of a host list: td_ids_check.h,
// td_copy_check.h; of a device list: the check kernel, td_list_check.h.)
#pragma once
#include <stddef.h>

#include <cstdio>

namespace td {

// A partial step (td_step_boards, td_step_boards_dev) on a handle whose settings rule it out:
// frame skip first, then random_agent = 0 with auto-reset.  True: refused, msg says why.
inline bool partial_step_refused(const char* fn, int frame_skip, int opp_np, int autoreset, char* msg, size_t n) {
  if (frame_skip > 1)
    std::snprintf(msg, n, "%s: not supported with frame skip (td_frame_skip() = %d); set td_set_frame_skip(h, 1) first", fn,
                  frame_skip);
  else if (opp_np && autoreset)
    std::snprintf(msg, n, "%s: not supported with random_agent = 0 and auto-reset on (the reset kernel behind a step "
                  "goes by done[] of every board, and an unnamed board's is stale)", fn);
  return frame_skip > 1 || (opp_np && autoreset);
}

// A device list's arguments against the handle's B boards, in this order: cap < 0, cap > B,
// cap == 0, a NULL list.  cap < 0 is refused whatever B is: it needs no handle, and every
// device-list call asks for that test alone (B = 0) in front of its handle's checks.
// have_lists: every list pointer of the call is there; lists: their names, for the message.
enum : int { LIST_ARGS_REFUSED = -1, LIST_ARGS_EMPTY = 0 /* the call returns 0, nothing enqueued */, LIST_ARGS_GO = 1 };
inline int list_args_check(const char* fn, int cap, int B, bool have_lists, const char* lists, char* msg, size_t n) {
  if (cap < 0) std::snprintf(msg, n, "%s: cap = %d is negative", fn, cap);
  else if (cap > B) std::snprintf(msg, n, "%s: cap = %d outside [0, %d] (the handle's boards)", fn, cap, B);
  else if (cap == 0) return LIST_ARGS_EMPTY;
  else if (!have_lists) std::snprintf(msg, n, "%s: %s is NULL with cap = %d", fn, lists, cap);
  else return LIST_ARGS_GO;
  return LIST_ARGS_REFUSED;
}

}  // namespace td
