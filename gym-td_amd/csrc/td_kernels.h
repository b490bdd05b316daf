// td_kernels.h -- interface between the C-ABI (td_capi.hip) and the kernel units: the kernels'
// arguments, the row lookups of the step, frame-skip and partial-step units (launched through
// td_step_launch.h) and the launch_* functions of td_reset.hip, td_mask.hip, td_mask_list.hip,
// td_sample.hip, td_copy.hip, td_copy_list.hip and td_list_check.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "td_common.h"
#include "td_list_check.h"
#include "../../include/tdstep.h"

namespace td {

// opponent hot record: [0] position, [1] lazy-twist boundary, [2] pre-drawn count,
// [3] position of the first pre-drawn output, [4..4+HOT_CACHE) pre-drawn tempered outputs for
// positions [3] .. [3]+count-1.  The large kernel refills them (from its position on) only
// when fewer than HOT_REFILL remain unused; the small kernels every step.
constexpr int HOT_CACHE = 8, HOT_REFILL = 8;
constexpr int HOT_WORDS = 4 + HOT_CACHE;

struct StepArgs {
  int B, L, mode, multi, difficulty, autoreset;
  int opp_np;           // random_agent=False: the built-in opponents draw from np_mt (auto-reset off)
  int small;            // 0 td_step_kernel, 1 td_step_kernel_small, 2 td_step_kernel_small2
  int obs_wt;           // small kernel: observation stores write-through (the batch's obs fits the MALL)
  TdHdr* hdr;
  double* en_lp;
  double* en_mg;
  uint32_t* en_inf;
  double* tw_cd;
  uint32_t* tw_inf;
  uint32_t* cells;
  uint32_t* opp_mt;     // [B][626] CPython-random MT words of the built-in opponent ([624..625] unused)
  uint32_t* opp_hot;    // [B][HOT_WORDS] its position, lazy-twist boundary, count and next 8 draws
  uint32_t* np_mt;      // [B][626] numpy-legacy state of the layout stream (TDGymBasic.np_random)
  // Staged next-episode layouts: a ring of NSLOT records per board (slot_words
  // words each, 128-B aligned).  Layout number n of a board's stream lives in slot
  // n % NSLOT with word 0 = slot_tag(n) once it is complete; lay_tail counts the
  // layouts drawn (written by the refill / reset kernels only), lay_head the
  // layouts consumed (written by the step / reset kernels only).
  uint32_t* nxt;        // [B][NSLOT][slot_words]
  uint32_t* lay_head;   // [B]
  uint32_t* lay_tail;   // [B]
  uint32_t* lay_claim;  // [B] 1 while a refill wave draws the board's layouts
  int slot_words;
  int refill_grp;       // boards scanned per refill wave per pass (refill_group)
  int refill_waves;     // waves per refill launch (each walks ceil(B / refill_grp / refill_waves) groups)
  int refill_walks;     // walks per board per refill launch (a draw resumes in the next launch)
  uint8_t* scratch;     // [B][scratch_stride] a pending layout draw: RoadResume header + generator arrays
  size_t scratch_stride;
  uint8_t* reset_fail;  // [B] reset kernel: road generation failed (board left unchanged)
  uint32_t* guard_to;   // [1] ring-guard claim waits that gave up (td_guard_timeouts)
  const int32_t* ovr_idx;   // reset kernel, td_reset_layouts: [B] record index in ovr_rec, or -1
  const uint32_t* ovr_rec;  // caller-supplied layout records (layout_words(L) each)
  const TdDevCfg* cfg;   // the current constant block (= cfgs + epoch)
  const TdDevCfg* cfgs;  // [NCFG] one block per paramConfig epoch (entities keep their epoch's values)
  int epoch;
  int frame_skip;  // board steps per launch (td_set_frame_skip), read by the skip kernels only (td_step_skip.h).
                   // In the 4 bytes of padding behind epoch: no field's kernarg offset moves, the struct
                   // keeps its size, and every other kernel compiles to the code it was.
  const int64_t* def_act;
  const int64_t* atk_act;
  float* obs;           // _Float16* with obs_f16
  double* reward;
  uint8_t* done;
  int64_t* real_def;
  int64_t* real_atk;
  int32_t* fail_def;
  int32_t* fail_atk;
  int8_t* win;
  uint8_t* allow_next;
  uint8_t* cooldowns;
  double* ep_return;
  int32_t* ep_len;
  double* ep_stats;  // [2]: finished episodes, sum of their returns (accumulated by the step kernel)
  td_episode_record* last_ep;  // [B]: each board's last finished episode (written on done)
  const uint8_t* reset_mask;  // reset kernel only (nullptr = all boards)
  int xcd_map;   // block i steps board xcd_board(i, B) (else board i)
  int edge_wt;   // observation lines shared with a neighbouring board: 2 plain, 1 write-through (write_obs_lines)
  int obs_f16;   // the observation is _Float16 [B][45][L][L] (td_set_obs_format): the *_f16 step kernels
  int obs_skip;  // obs is the retained buffer and holds every board's last observation (td_retain_obs): the
                 // step may leave the windows of clean dirty classes unwritten (write_obs_lines)
};
static_assert(offsetof(StepArgs, frame_skip) == offsetof(StepArgs, epoch) + 4 && offsetof(StepArgs, def_act) % 8 == 0 &&
                  offsetof(StepArgs, def_act) == offsetof(StepArgs, epoch) + 8,
              "frame_skip lies in the padding behind epoch");
constexpr int NXCD = 8;  // XCDs of an MI355X: block i runs on XCD i % 8

// The XCD-contiguous board map: block i (XCD i % 8, slot i / 8) steps board
// prefix(i % 8) + i / 8, so XCD x steps the contiguous range of boards after those of
// XCDs 0 .. x-1.  Neighbouring boards then share an L2: the lines of the small per-board
// arrays (header, hot record, reward, done, info) and the observation lines two boards
// share are written whole by one XCD instead of in pieces by several.
__host__ __device__ inline int xcd_board(int i, int B) {
  const int x = i & (NXCD - 1), q = B / NXCD, r = B % NXCD;
  return x * q + (x < r ? x : r) + i / NXCD;
}

// One row of the launch table of the step, frame-skip and partial-step kernels
// (td_step_launch.h: selection, launch, occupancy, display name).
constexpr int kNoScan = -1;  // scan of a family whose kernels have no SCAN parameter (the skip kernels)
struct KernelRow {
  const void* fn;
  int threads;       // per block: 64, or 128 for the two-wave step kernel
  const char* name;  // the kernel template, and its arguments (filled in by select_row):
  int lt = 0, mode = 0, scan = 0;
};
// What a kernel unit exports: its row for a.L, a.mode and a.multi.  The step units
// (td_step.hip, td_step_f16.hip) by kind: 0 large, 1 small, 2 small2 (StepArgs::small); the
// frame-skip units (td_step_skip.hip, td_step_skip_f16.hip) and the partial-step units
// (td_step_sel.hip, td_step_sel_f16.hip) have one kernel per row.
KernelRow step_row_f32(const StepArgs& a, int kind);
KernelRow step_row_f16(const StepArgs& a, int kind);
KernelRow skip_row_f32(const StepArgs& a);
KernelRow skip_row_f16(const StepArgs& a);
KernelRow sel_row_f32(const StepArgs& a);
KernelRow sel_row_f16(const StepArgs& a);
// The partial step whose list, count and verdict are read from device memory
// (td_step_boards_dev; td_step_list.hip, td_step_list_f16.hip): one kernel per row, as sel_row_*.
KernelRow list_row_f32(const StepArgs& a);
KernelRow list_row_f16(const StepArgs& a);

// What a playout kernel takes beside its StepArgs (td_playout, td_playout_boards[_dev];
// td_playout.h): the sampler's call (td_sample.h: key0 = sample_sm(seed), so sub-step j's key is
// sample_sm(key0 + ticket + j)), the entries it serves and the outputs a step does not have.
// StepArgs::frame_skip carries the number of sub-steps; its output pointers carry the rest.
struct PlayoutArgs {
  uint64_t key0;
  uint64_t ticket;
  uint32_t def_idle, atk_idle;
  // ids == nullptr: every board (entry i is board i).  Else td_sample_kernel's contract: boards
  // ids[0 .. cap) where verdict == nullptr, else ids[0 .. *count) (count == nullptr: cap) unless
  // the check kernel launched in front refused the list.
  const int32_t* ids;
  int cap;
  const int32_t* count;
  const td_list_status* verdict;
  int32_t* steps_run;    // [B] sub-steps executed, or nullptr
  int64_t* first_def;    // [B] the defender's action of sub-step 0, or nullptr
  int64_t* first_atk;    // [B][3][8] the attacker's, or nullptr
};
// The playout unit's row (td_playout.hip): one kernel per (side, mode), no SCAN parameter.
KernelRow playout_row(const StepArgs& a);

// What a probe kernel takes beside its StepArgs (td_probe, td_probe_boards[_dev]; td_probe.h):
// the playout's call and entries, and the replicas per entry.  Replica r of board b is the playout
// at ticket p.ticket + r * steps (steps: StepArgs::frame_skip), and its outputs are row
// b * reps + r of [B][reps] buffers: StepArgs::reward / done / win and p's steps_run, first_def,
// first_atk.  Every other output pointer of the StepArgs is unused.
struct ProbeArgs {
  PlayoutArgs p;
  int reps;
};
// The probe unit's row (td_probe.hip): one kernel per (side, mode), no SCAN parameter.
KernelRow probe_row(const StepArgs& a);

// TDGymBasic.reset for the boards in a.reset_mask (nullptr = all); failures in a.reset_fail.
hipError_t launch_reset(const StepArgs& a, hipStream_t s);
// random_agent=False with auto-reset: reset the boards the step just finished (a.done),
// drawing their layouts from the shared numpy stream now (same stream, after the step).
hipError_t launch_autoreset(const StepArgs& a, hipStream_t s);
// Config epochs referred to by live enemies / towers: bit e of used[NCFG / 32] (zeroed by the caller).
hipError_t launch_cfg_usage(const StepArgs& a, uint32_t* used, hipStream_t s);
// Draw staged layouts for every board whose ring has a free slot: a side-stream refill
// (guard = 0), or the ring guard on the step stream (guard = G: every ring below G
// layouts filled to G, draws run to the end; td_reset.hip td_refill_kernel).
hipError_t launch_refill(const StepArgs& a, hipStream_t s, int guard = 0);
// The built-in opponent (side 0: random_enemy_lv<level>, 1: random_tower_lv<level>)
// on the boards in a.reset_mask (nullptr = all).
hipError_t launch_opponent(const StepArgs& a, int side, int level, hipStream_t s);
// Board copy (td_copy_boards; td_copy.hip): boards pairs[n + i] become copies of boards pairs[i],
// i in [0, n), n >= 1; `pairs` is device memory, the ids validated by the caller.  With a.obs the
// destinations' observation rows are written whole in the format a.obs_f16.
// ev0 / ev1: optional timing events bound to the kernel's dispatch, as launch_step's.
hipError_t launch_copy(const StepArgs& a, const int32_t* pairs, int n, hipStream_t s, hipEvent_t ev0 = nullptr,
                       hipEvent_t ev1 = nullptr);
// The same copy for a device-resident list (td_copy_boards_dev): boards dst[i] become copies of
// boards src[i] for i < *count (count == nullptr: cap), unless verdict->code says the list was
// refused (td_list_check.hip, launched in front): then no wave reads or writes anything of any
// board.  One block per entry of cap.
hipError_t launch_copy_list(const StepArgs& a, const int32_t* src, const int32_t* dst, int cap, const int32_t* count,
                            const td_list_status* verdict, hipStream_t s, hipEvent_t ev0 = nullptr,
                            hipEvent_t ev1 = nullptr);
// The check of a device-resident list (td_list_check.hip): one thread per entry of a.cap >= 1.
hipError_t launch_list_check(const ListCheckArgs& a, hipStream_t s);

// What the mask and sample kernels read of the boards, filled from the handle in one place
// (td_capi.hip board_view): the header, the cell words (map[6] in bits 24-31), the tower words
// and the current constant block.  The first member of both kernels' arguments.
struct BoardView {
  int B, L, multi;
  int xcd_map;           // block i serves board xcd_board(i, B) (else board i), as the step
  const TdHdr* hdr;
  const uint32_t* tw_inf;
  const uint32_t* cells;
  const TdDevCfg* cfg;   // the current constant block
};

// Legal-action masks of the boards' present state (td_action_mask; td_mask.hip): which
// action the next step would execute.  Reads the view; writes only the outputs.
struct MaskArgs {
  BoardView v;
  uint8_t* def_mask;     // [B][def_pitch] or nullptr
  uint8_t* def_code;     // [B][def_pitch] or nullptr
  uint8_t* atk_mask;     // [B][3][5] or nullptr
  size_t def_pitch;      // bytes per board: >= 6 L^2 + 1 (discrete), 6 L^2 (multi-action)
};
constexpr size_t kMaskMaxPitch = 1u << 16;
hipError_t launch_mask(const MaskArgs& a, hipStream_t s);
// The same masks for the boards a list names, every other row left as it is
// (td_action_mask_boards[_dev]; td_mask_list.hip): boards ids[0 .. cap) of device memory where
// verdict == nullptr (the ids validated by the caller); else boards ids[0 .. *count) (count ==
// nullptr: cap), unless verdict->code says the check kernel launched in front refused the list:
// then nothing is read of any board and nothing is written.  One wave per entry of cap >= 1,
// kMaskListWaves entries per workgroup (TD_MASK_LIST_WAVES: a build-time measurement knob).
#ifndef TD_MASK_LIST_WAVES
#define TD_MASK_LIST_WAVES 4
#endif
constexpr int kMaskListWaves = TD_MASK_LIST_WAVES;
static_assert(kMaskListWaves >= 1 && kMaskListWaves <= 8, "waves of one workgroup (their LDS rows: 64 KB)");
hipError_t launch_mask_list(const MaskArgs& a, const int32_t* ids, int cap, const int32_t* count,
                            const td_list_status* verdict, hipStream_t s);

// One uniformly drawn legal action per side and board (td_sample_actions[_boards[_dev]];
// td_sample.hip): reads the view, writes only the outputs.
struct SampleArgs {
  BoardView v;
  int64_t* def_act;      // [B] or [B][6][L][L], or nullptr
  int64_t* atk_act;      // [B][3][8] or nullptr
  int32_t* def_count;    // [B] or nullptr
  int32_t* atk_count;    // [B] or nullptr
  uint64_t key;          // sample_key(seed, ticket) (td_sample.h)
  uint32_t def_idle, atk_idle;
};
// the kernarg offsets the kernels were built with: the view in front, the outputs behind it
static_assert(offsetof(BoardView, xcd_map) == 12 && offsetof(BoardView, hdr) == 16 && offsetof(BoardView, tw_inf) == 24 &&
                  offsetof(BoardView, cells) == 32 && offsetof(BoardView, cfg) == 40 && sizeof(BoardView) == 48,
              "BoardView's layout");
static_assert(offsetof(MaskArgs, v) == 0 && offsetof(MaskArgs, def_mask) == 48 && offsetof(MaskArgs, def_pitch) == 72 &&
                  sizeof(MaskArgs) == 80, "MaskArgs' layout");
static_assert(offsetof(SampleArgs, v) == 0 && offsetof(SampleArgs, def_act) == 48 && offsetof(SampleArgs, key) == 80 &&
                  offsetof(SampleArgs, atk_idle) == 92 && sizeof(SampleArgs) == 96, "SampleArgs' layout");
constexpr int kSampleWaves = 4;  // entries (waves) per workgroup, as kMaskListWaves
// ids == nullptr: every board (cap = B, entry i is board i); else td_mask_list_kernel's contract:
// boards ids[0 .. cap) where verdict == nullptr, else ids[0 .. *count) unless the check kernel
// launched in front refused the list.  One wave per entry of cap >= 1.
hipError_t launch_sample(const SampleArgs& a, const int32_t* ids, int cap, const int32_t* count,
                         const td_list_status* verdict, hipStream_t s);

// One legal action per side and board drawn in proportion to the caller's weights
// (td_sample_weighted[_boards[_dev]]; td_sample_w.hip): reads the view and the weight rows, writes
// only the outputs.  Discrete defender actions only (the call refuses the rest).
struct SampleWArgs {
  BoardView v;
  int64_t* def_act;      // [B] or nullptr
  int64_t* atk_act;      // [B][3][8] or nullptr
  const float* def_w;    // [B][def_pitch] floats, 4-B aligned; there where def_act is
  const float* atk_w;    // [B][13]; there where atk_act is
  uint64_t* def_mass;    // [B][2] (m(chosen), S) or nullptr
  uint64_t* atk_mass;    // [B][2] or nullptr
  size_t def_pitch;      // floats per board: >= 6 L^2 + 1
  uint64_t key;          // sample_key(seed, ticket) (td_sample.h)
};
static_assert(offsetof(SampleWArgs, v) == 0 && offsetof(SampleWArgs, def_act) == 48 && offsetof(SampleWArgs, key) == 104 &&
                  sizeof(SampleWArgs) == 112, "SampleWArgs' layout");
constexpr size_t kSampleWMaxPitch = 1u << 16;  // floats
// ids, cap, count, verdict: launch_sample's.  kSampleWaves entries per workgroup.
hipError_t launch_sample_weighted(const SampleWArgs& a, const int32_t* ids, int cap, const int32_t* count,
                                  const td_list_status* verdict, hipStream_t s);

// Staged layouts per board: sixteen episodes of slack for the side refills, and the
// ring guard (td_refill_kernel) needs to run only every NSLOT - 1 steps.  (NSLOT = 4 with
// a guard every 3rd step: +4 % / +7-9 % per step at 8,192 / 4,096 boards, profiles/r03/s13.)
constexpr int NSLOT = 16;
__host__ __device__ inline uint32_t slot_tag(uint32_t n) { return 0x80000000u | (n & 0x7fffffffu); }
__host__ __device__ inline int slot_words(int L) { return (8 + L * L + 31) & ~31; }
// Boards scanned per refill wave when a refill launch has `waves` waves (at most 64:
// one ballot per wave).
__host__ __device__ inline int refill_group(int B, int waves) {
  const int g = (B + waves - 1) / waves;
  return g < 1 ? 1 : (g > 64 ? 64 : g);
}

constexpr int kRoadAttempts = 1000;  // bound of each create_road_v2 retry loop (reference: unbounded)
constexpr int kLayoutRetries = 64;   // auto-reset: failing draws skipped before giving up

constexpr uint64_t kTakeSpinTicks = 100000000ull;  // 1 s of the 100-MHz clock: longest wait for a refill wave

}  // namespace td
