// td_call_check.h -- what the list calls refuse of the handle's settings and of a device list's
// arguments, and the sampler of its io, each written once.  Plain C++, no HIP: functions of the handle's ints that write a
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

// What td_sample_actions and its list forms refuse of their io, in this order: a NULL io, a bad
// size / abi word, a NULL handle, no action output wanted, an output or count for a side the
// mode lacks.  The caller fills in the pointers' presence only once the two header words match
// (a struct of another layout is not read past them).  mode: 0 TD-def, 1 TD-atk, 2 TD-2p.
struct SampleIoSeen {
  bool io = false;                // io != NULL
  unsigned size = 0, abi = 0;     // its two header words
  bool handle = false;            // h != NULL
  int mode = 0;                   // the handle's
  bool def_act = false, atk_act = false, def_count = false, atk_count = false;  // != NULL
};
inline bool sample_io_header_ok(const SampleIoSeen& v, unsigned want_size, int want_abi) {
  return v.io && v.size == want_size && v.abi == (unsigned)want_abi;
}
inline bool sample_io_refused(const char* fn, const SampleIoSeen& v, unsigned want_size, int want_abi, char* msg, size_t n) {
  if (!v.io) std::snprintf(msg, n, "%s: NULL io", fn);
  else if (!sample_io_header_ok(v, want_size, want_abi))
    std::snprintf(msg, n, "%s: td_sample_io has size %u / abi %u, this library expects size %u / abi %d "
                  "(call td_sample_io_init)", fn, v.size, v.abi, want_size, want_abi);
  else if (!v.handle) std::snprintf(msg, n, "%s: NULL handle", fn);
  else if (!v.def_act && !v.atk_act) std::snprintf(msg, n, "%s: no action output wanted (def_act and atk_act are NULL)", fn);
  else if ((v.def_act || v.def_count) && v.mode == 1)
    std::snprintf(msg, n, "%s: TD-atk has no defender side (def_act / def_count)", fn);
  else if ((v.atk_act || v.atk_count) && v.mode == 0)
    std::snprintf(msg, n, "%s: TD-def has no attacker side (atk_act / atk_count)", fn);
  else return false;
  return true;
}

// What td_sample_weighted and its list forms refuse of their io, in this order: a NULL io, a bad
// size / abi word, a NULL handle, no action output wanted, any pointer of a side the mode lacks, an
// action output without its weights or a mass without its action, a weight pointer that is no
// multiple of 4, a pitch outside [row, max_pitch] (0: the row), the defender side on a multi-action
// handle (its attacker side is served).  The caller fills in everything behind the header words
// only once they match and there is a handle.  row: 6 L^2 + 1 floats.
struct SampleWIoSeen {
  bool io = false;                // io != NULL
  unsigned size = 0, abi = 0;     // its two header words
  bool handle = false;            // h != NULL
  int mode = 0, multi = 0;        // the handle's
  bool def_act = false, atk_act = false, def_w = false, atk_w = false, def_mass = false, atk_mass = false;  // != NULL
  bool def_w_aligned = true, atk_w_aligned = true;  // the address is a multiple of 4
  size_t pitch = 0, row = 0;      // io->def_w_pitch; the handle's row
};
inline bool sample_w_io_header_ok(const SampleWIoSeen& v, unsigned want_size, int want_abi) {
  return v.io && v.size == want_size && v.abi == (unsigned)want_abi;
}
inline bool sample_w_io_refused(const char* fn, const SampleWIoSeen& v, unsigned want_size, int want_abi, size_t max_pitch,
                                char* msg, size_t n) {
  if (!v.io) std::snprintf(msg, n, "%s: NULL io", fn);
  else if (!sample_w_io_header_ok(v, want_size, want_abi))
    std::snprintf(msg, n, "%s: td_sample_w_io has size %u / abi %u, this library expects size %u / abi %d "
                  "(call td_sample_w_io_init)", fn, v.size, v.abi, want_size, want_abi);
  else if (!v.handle) std::snprintf(msg, n, "%s: NULL handle", fn);
  else if (!v.def_act && !v.atk_act) std::snprintf(msg, n, "%s: no action output wanted (def_act and atk_act are NULL)", fn);
  else if ((v.def_act || v.def_w || v.def_mass) && v.mode == 1)
    std::snprintf(msg, n, "%s: TD-atk has no defender side (def_act / def_w / def_mass)", fn);
  else if ((v.atk_act || v.atk_w || v.atk_mass) && v.mode == 0)
    std::snprintf(msg, n, "%s: TD-def has no attacker side (atk_act / atk_w / atk_mass)", fn);
  else if (v.def_act && !v.def_w) std::snprintf(msg, n, "%s: def_act without its weights (def_w is NULL)", fn);
  else if (v.atk_act && !v.atk_w) std::snprintf(msg, n, "%s: atk_act without its weights (atk_w is NULL)", fn);
  else if (v.def_mass && !v.def_act) std::snprintf(msg, n, "%s: def_mass without its action (def_act is NULL)", fn);
  else if (v.atk_mass && !v.atk_act) std::snprintf(msg, n, "%s: atk_mass without its action (atk_act is NULL)", fn);
  else if (!v.def_w_aligned) std::snprintf(msg, n, "%s: def_w is no multiple of 4 (float32 rows)", fn);
  else if (!v.atk_w_aligned) std::snprintf(msg, n, "%s: atk_w is no multiple of 4 (float32 rows)", fn);
  else if (v.def_act && v.pitch != 0 && (v.pitch < v.row || v.pitch > max_pitch))
    std::snprintf(msg, n, "%s: def_w_pitch %zu outside [%zu, %zu] (6 L^2 + 1 floats per row)", fn, v.pitch, v.row, max_pitch);
  else if (v.def_act && v.multi)
    std::snprintf(msg, n, "%s: the defender side is not supported with multi-action (one discrete action is "
                  "sampled); the attacker side is", fn);
  else return false;
  return true;
}

// What td_playout and its list forms refuse of their io and of the handle's settings, in this
// order: a NULL io, a bad size / abi word, a NULL handle, steps outside [1, max_steps], a missing
// reward or done, a first action for a side the mode lacks, a multi-action handle, random_agent
// = 0.  The caller fills in everything behind the header words only once they match, and the
// handle's settings only where there is a handle.  mode: 0 TD-def, 1 TD-atk, 2 TD-2p.
// td_probe and its list forms refuse the same in the same order, with reps outside [1, max_reps]
// behind the steps: `probe` names the io and the limit (nullptr: the playout's io, no replicas).
struct PlayoutIoSeen {
  bool io = false;                // io != NULL
  unsigned size = 0, abi = 0;     // its two header words
  bool handle = false;            // h != NULL
  int steps = 0;                  // io->steps
  bool reward = false, done = false, first_def = false, first_atk = false;  // != NULL
  int mode = 0, multi = 0, opp_np = 0;  // the handle's
  int reps = 1;                   // io->reps (a probe's)
};
struct ProbeIoLimit {
  int max_reps;  // TD_MAX_PROBE_REPS
};
inline bool playout_io_header_ok(const PlayoutIoSeen& v, unsigned want_size, int want_abi) {
  return v.io && v.size == want_size && v.abi == (unsigned)want_abi;
}
inline bool playout_io_refused(const char* fn, const PlayoutIoSeen& v, unsigned want_size, int want_abi, int max_steps,
                               char* msg, size_t n, const ProbeIoLimit* probe = nullptr) {
  const char* const io = probe ? "td_probe_io" : "td_playout_io";
  const char* const what = probe ? "probe" : "playout";
  if (!v.io) std::snprintf(msg, n, "%s: NULL io", fn);
  else if (!playout_io_header_ok(v, want_size, want_abi))
    std::snprintf(msg, n, "%s: %s has size %u / abi %u, this library expects size %u / abi %d "
                  "(call %s_init)", fn, io, v.size, v.abi, want_size, want_abi, io);
  else if (!v.handle) std::snprintf(msg, n, "%s: NULL handle", fn);
  else if (v.steps < 1 || v.steps > max_steps)
    std::snprintf(msg, n, "%s: steps = %d outside [1, %d] (TD_MAX_PLAYOUT_STEPS)", fn, v.steps, max_steps);
  else if (probe && (v.reps < 1 || v.reps > probe->max_reps))
    std::snprintf(msg, n, "%s: reps = %d outside [1, %d] (TD_MAX_PROBE_REPS)", fn, v.reps, probe->max_reps);
  else if (!v.reward || !v.done) std::snprintf(msg, n, "%s: reward and done are required", fn);
  else if (v.first_def && v.mode == 1) std::snprintf(msg, n, "%s: TD-atk has no defender side (first_def)", fn);
  else if (v.first_atk && v.mode == 0) std::snprintf(msg, n, "%s: TD-def has no attacker side (first_atk)", fn);
  else if (v.multi)
    std::snprintf(msg, n, "%s: not supported with multi-action (the %s samples one discrete action per side and "
                  "sub-step)", fn, what);
  else if (v.opp_np)
    std::snprintf(msg, n, "%s: not supported with random_agent = 0 (the built-in opponent would draw from the layout "
                  "stream inside the launch)", fn);
  else return false;
  return true;
}

}  // namespace td
