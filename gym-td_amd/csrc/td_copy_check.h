// td_copy_check.h -- the host-side check of td_copy_boards' index arrays.  Plain C++, no HIP:
// td_capi.hip calls it before anything is enqueued, and scripts/copy_check_host.cpp runs it
// alone under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <vector>

namespace td {

enum : int {
  COPY_OK = 0,
  COPY_BAD_COUNT,  // n < 0 or n > B
  COPY_NULL,       // n > 0 with a NULL array
  COPY_RANGE,      // an id outside [0, B)
  COPY_DST_TWICE,  // a board named twice in dst
  COPY_OVERLAP,    // a board named in both src and dst (the result would depend on pair order)
};

// role: B bytes of scratch, all zero on entry and all zero again on return (only the entries
// of the ids named are touched).  A board repeated in src is fine: one root, many children.
// On a refusal msg says which pair, and nothing else was written.
inline int copy_check(const int32_t* src, const int32_t* dst, int n, int B, std::vector<uint8_t>& role, char* msg,
                      size_t cap) {
  if (n < 0 || n > B) {
    std::snprintf(msg, cap, "n = %d outside [0, %d] (the handle's boards)", n, B);
    return COPY_BAD_COUNT;
  }
  if (n == 0) return COPY_OK;
  if (!src || !dst) {
    std::snprintf(msg, cap, "src / dst is NULL with n = %d", n);
    return COPY_NULL;
  }
  if (role.size() != (size_t)B) role.assign((size_t)B, 0);
  // Three passes over the ids: range and the sources' marks, the destinations, the clean-up.
  int rc = COPY_OK, at = 0, marked = 0;
  for (; marked < n; ++marked) {
    const int32_t sb = src[marked], db = dst[marked];
    if (sb < 0 || sb >= B || db < 0 || db >= B) break;
    role[(size_t)sb] = 1;  // 1 a source, 2 a destination
  }
  if (marked < n) {
    for (int i = 0; i < marked; ++i) role[(size_t)src[i]] = 0;
    std::snprintf(msg, cap, "pair %d: src %d / dst %d outside [0, %d)", marked, src[marked], dst[marked], B);
    return COPY_RANGE;
  }
  for (int i = 0; i < n && rc == COPY_OK; ++i) {
    uint8_t& r = role[(size_t)dst[i]];
    if (r == 1) { rc = COPY_OVERLAP; at = i; }
    else if (r == 2) { rc = COPY_DST_TWICE; at = i; }
    else r = 2;
  }
  for (int i = 0; i < n; ++i) role[(size_t)src[i]] = role[(size_t)dst[i]] = 0;
  if (rc == COPY_OVERLAP)
    std::snprintf(msg, cap, "pair %d: board %d is a source and a destination (the result would depend on pair order)", at,
                  dst[at]);
  else if (rc == COPY_DST_TWICE)
    std::snprintf(msg, cap, "pair %d: board %d is named twice in dst", at, dst[at]);
  return rc;
}

}  // namespace td
