// td_ids_check.h -- the host-side check of td_step_boards' board list.  Plain C++, no HIP:
// td_capi.hip calls it before anything is enqueued, and scripts/ids_check_host.cpp runs it
// alone under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <vector>

namespace td {

enum : int {
  IDS_OK = 0,
  IDS_BAD_COUNT,  // n < 0 or n > B
  IDS_NULL,       // n > 0 with a NULL array
  IDS_RANGE,      // an id outside [0, B)
  IDS_TWICE,      // a board named twice (two waves would step one board)
};

// seen: B bytes of scratch, all zero on entry and all zero again on return (only the entries
// of the ids named are touched).  One pass marks the ids up to the first bad one, a second
// clears the marks.  On a refusal msg says which entry, and nothing else was written.
inline int ids_check(const int32_t* ids, int n, int B, std::vector<uint8_t>& seen, char* msg, size_t cap) {
  if (n < 0 || n > B) {
    std::snprintf(msg, cap, "n = %d outside [0, %d] (the handle's boards)", n, B);
    return IDS_BAD_COUNT;
  }
  if (n == 0) return IDS_OK;
  if (!ids) {
    std::snprintf(msg, cap, "boards is NULL with n = %d", n);
    return IDS_NULL;
  }
  if (seen.size() != (size_t)B) seen.assign((size_t)B, 0);
  int rc = IDS_OK, marked = 0;
  for (; marked < n; ++marked) {
    const int32_t b = ids[marked];
    if (b < 0 || b >= B) { rc = IDS_RANGE; break; }
    if (seen[(size_t)b]) { rc = IDS_TWICE; break; }
    seen[(size_t)b] = 1;
  }
  for (int i = 0; i < marked; ++i) seen[(size_t)ids[i]] = 0;
  if (rc == IDS_RANGE) std::snprintf(msg, cap, "entry %d: board %d outside [0, %d)", marked, ids[marked], B);
  else if (rc == IDS_TWICE) std::snprintf(msg, cap, "entry %d: board %d is named twice", marked, ids[marked]);
  return rc;
}

}  // namespace td
