// td_capi.hip -- the C-ABI (include/tdstep.h): handle, HBM buffers, launches.
//
// Everything per board lives on the device: board records, both RNG streams
// (layouts: numpy-legacy MT19937; built-in opponent: CPython MT19937) and the
// staged next-episode layout.  Layouts are generated on the device
// (td_refill_kernel / td_reset_kernel), so the step loop has no host work.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/tdstep.h"
#include "../../include/td_diag.h"
#include "../../include/td_diag_retained.h"
#include "td_call_check.h"
#include "td_cfg_check.h"
#include "td_copy_check.h"
#include "td_ids_check.h"
#include "td_kernel_choice.h"
#include "td_kernels.h"
#include "td_layout.h"
#include "td_obs_ledger.h"
#include "td_rng.h"
#include "td_sample.h"
#include "td_state_rec.h"
#include "td_step_launch.h"
#include "td_upgrade_step.h"

using namespace td;

namespace {

thread_local std::string g_err;

int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}

#define HIP_OK(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return fail("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// Steps between refill launches (td_set_refill_interval).  Every 16th step instead of
// every 4th: 23.7 / 36.3 / 208.3 vs 24.9 / 37.1 / 209.2 us per step at 4,096 / 8,192 /
// 65,536 boards, no ring dry over 5,000 steps, the GPU suite green (profiles/r02/s44).
// Every launch is ordered behind the step stream (start_refill):
// refills left unordered between steps ran 4-8 % faster at 4,096 / 8,192 boards, but a
// step that finds a ring empty then has no refill beside it to wait for: under load a
// board missed its layout (test_autoreset_under_load, profiles/r02/s43_unordered).
// With rings of 16 and the ring guard, every 64th step: 34.3 / 21.5 us per step at
// 8,192 / 4,096 boards vs 34.8 / 22.2-22.75 at every 16th, +-0 at 65,536; no refill and
// no guard at all (rings draining, not a product setting): 33.1-33.8 / 20.0
// (profiles/r03/s23).
constexpr int kRefillEvery = 64;
constexpr int kRefillWaves = 1024;
// A pending draw advances 3 walks per step of refill interval (48 per launch at 16): the
// fewer walks a refill wave runs per launch, the less it holds a wave slot the next
// step's waves need (8,192 boards, a refill every 4th step: 37.9 us per step at 48 walks, 36.5 at 12, 36.6 at 4,
// 36.9 at 1; 34.3 without refills, profiles/r02/s21_session.log).
constexpr int kWalksPerStep = 3;
// The ring guard (td_reset.hip td_refill_kernel, guard = G) runs on the step stream before
// every G-th step and fills every ring below G layouts to G: a board consumes at most one
// layout per step, so none of the next G steps finds a ring empty, whatever the refill
// cadence.  G = NSLOT - 1: a ring the side refills keep full only falls below it when a
// board finishes two episodes between two refills, so the guard rarely draws (G = NSLOT
// made it draw for every board that finished one: 8,192 boards 78 vs 35 us per step,
// profiles/r03/s12); a launch is then a scan of the rings, paid every G steps.
constexpr int kGuardEvery = NSLOT - 1;
constexpr int kSideStreams = 2;  // refill streams: one stuck on a long draw does not stall the next (the HIP
                                 // runtime has 4 hardware queues per process; the step stream needs one)
constexpr int kIdSlots = 4;      // td_copy_boards, td_step_boards: id uploads in flight before a call waits for the oldest
// The strings the kernel-name accessors hand out: one slot each, so a name stays valid until
// its own accessor is called again (kept_name).
enum { NAME_STEP, NAME_SEL, NAME_LIST, NAME_MASK_LIST, NAME_SAMPLE, NAME_PLAYOUT, NAME_SAMPLE_W, NAME_PROBE, NAME_SLOTS };

}  // namespace

struct td_handle {
  int L = 0, NC = 0, B = 0, mode = 0, multi = 0, difficulty = 1, device = 0, autoreset = 1;
  int opp_np = 0;  // random_agent=False
  KernelChoice kernel;        // the step kernels of a full and of a skipping launch (td_kernel_choice.h)
  int resident[2][2] = {};    // [format][waves - 1]: boards resident at once (step_resident_boards)
  int obs_fmt = TD_OBS_F32;   // td_set_obs_format: the element every obs pointer is taken to hold
  int frame_skip = 1;         // td_set_frame_skip: board steps per td_step (> 1: the skip kernel is launched)
  std::string names[NAME_SLOTS];  // td_step_kernel_name, td_step_boards[_dev]_kernel_name, td_action_mask_boards_kernel_name, td_sample_actions_kernel_name, td_playout_kernel_name, td_sample_weighted_kernel_name, td_probe_kernel_name
  int lw = 0;  // layout record words
  size_t scratch_stride = 0;
  TdDevCfg dcfg;
  TdDevCfg* d_cfg = nullptr;  // [NCFG]: one constant block per paramConfig epoch
  int epoch = 0;              // the current block
  int cfg_fresh = 1;          // blocks [cfg_fresh, NCFG) never used yet
  TdHdr* d_hdr = nullptr;
  double *d_en_lp = nullptr, *d_en_mg = nullptr, *d_tw_cd = nullptr;
  uint32_t *d_en_inf = nullptr, *d_tw_inf = nullptr, *d_cells = nullptr, *d_opp = nullptr, *d_np = nullptr;
  uint32_t* d_hot = nullptr;  // opponent hot record [B][HOT_WORDS]
  uint32_t *d_nxt = nullptr, *d_stage = nullptr;  // staged-layout rings [B][NSLOT][slot_words]; caller records
  uint32_t *d_lay_head = nullptr, *d_lay_tail = nullptr, *d_lay_claim = nullptr;  // rings (td_kernels.h)
  int32_t* d_ovr_idx = nullptr;                           // td_reset_layouts: [B] index into d_stage or -1
  uint8_t *d_scratch = nullptr, *d_mask = nullptr, *d_fail = nullptr;
  int stage_cap = 0;
  double* d_epstats = nullptr;   // [2] finished episodes, sum of their returns
  td_episode_record* d_lastep = nullptr;  // [B] each board's last finished episode
  // Layout refills run on kSideStreams side streams in turn; the step stream never
  // waits for them (the rings give every board NSLOT episodes of slack, and
  // per-board claims keep concurrent refills apart).
  hipStream_t side[kSideStreams] = {};
  hipEvent_t ev_main = nullptr;  // orders a refill after a reset kernel (system-scope fence)
  hipEvent_t ev_step = nullptr;  // orders a refill after the previous step (no system-scope fence)
  int next_side = 0;
  int refill_every = kRefillEvery;  // 0: no refill launches (td_set_refill_interval)
  int refill_waves = kRefillWaves;  // waves per refill launch
  int guard_every = kGuardEvery;  // ring guard cadence
  int since_guard = kGuardEvery;  // steps launched since the last ring guard (>= guard_every: guard first)
  // td_kernel_timing: event pairs bound to the next `tev_cap` step-kernel dispatches
  std::vector<hipEvent_t> tev;
  int tev_cap = 0, tev_n = 0, tev_every = 1;
  long long tev_from = 0;  // h->steps when td_kernel_timing was called
  long long steps = 0;
  std::vector<int32_t> last_reset_failed;
  uint32_t* d_guard_to = nullptr;  // [1] ring-guard claim waits that gave up (td_guard_timeouts)
  int xcd_map = 1;  // XCD-contiguous board map (td_kernels.h xcd_board; td_set_store_policy)
  int edge_wt = 2;  // observation lines shared with a neighbour: plain write-back stores, merged in the XCD's L2
                    // (1.088x vs 1.093x the algorithmic bytes at 65,536 boards, step time +-0, profiles/r04/s20);
                    // 1: write-through (sc1), the reference form of tests/test_gpu_store_policy.py
  ObsLedger ledger;  // td_retain_obs: the retained buffer and what is known of it (td_obs_ledger.h)
  // td_copy_boards, td_step_boards: the caller's id arrays travel through kIdSlots pinned slots of 2 B ids
  // in turn (allocated by td_create), each to d_pairs on the call's stream; a slot is
  // written again only once the event behind its last upload has passed (upload_ids)
  int32_t* id_stage = nullptr;  // pinned host [kIdSlots][2 B]
  int32_t* d_pairs = nullptr;   // [2 B]: a copy's sources, then its destinations; or a partial step's boards
  hipEvent_t id_ev[kIdSlots] = {};
  int id_next = 0;
  std::vector<uint8_t> id_role;  // [B] copy_check's scratch, and ids_check's: all zero between calls
  // td_step_boards_dev, td_copy_boards_dev (td_list_check.h): the check kernel's per-board mark
  // words, the record its verdict goes to, and the serial of the next call that launches
  uint32_t* d_list_marks = nullptr;  // [B]
  ListState* d_list = nullptr;       // [1]
  long long list_calls = 0;
};

namespace {

void build_dev_cfg(const td_config& c, TdDevCfg& d) {
  std::memset(&d, 0, sizeof d);
  for (int t = 0; t < 4; ++t)
    for (int l = 0; l < 2; ++l) {
      d.e_lp[t][l] = c.enemy_LP[t][l];
      d.e_speed[t][l] = c.enemy_speed[t][l];
      d.e_def[t][l] = c.enemy_defense[t][l];
      d.e_cost[t][l] = c.enemy_cost[t][l];
      d.t_atk[t][l] = c.tower_attack[t][l];
      d.t_rge[t][l] = c.tower_range[t][l];
      d.t_dmg[t][l] = c.tower_splash_range[t][l];
      d.t_price[t][l] = c.tower_cost[t][l];
    }
  // Tower attributes after create_tower / upgrade_tower (TDElements.py:134-170):
  // lvup(atk, rge, dmgrge, intv=tower_cost[t][l], cost += tower_attack_interval[t][l]).
  for (int t = 0; t < 4; ++t) {
    d.t_intv[t][0] = c.tower_attack_interval[t][0];
    d.t_intv[t][1] = c.tower_cost[t][1];
    d.t_addcost[t][0] = 0.0;
    d.t_addcost[t][1] = c.tower_attack_interval[t][1];
  }
  d.destruct_return = c.tower_destruct_return;
  d.frozen_ratio = c.frozen_ratio;
  d.max_cost = c.max_cost;
  d.reward_kill = c.reward_kill;
  d.penalty_leak = c.penalty_leak;
  d.reward_time = c.reward_time;
  d.atk_init_rate = c.attacker_cost_init_rate;
  d.atk_final_rate = c.attacker_cost_final_rate;
  d.def_rate = c.defender_cost_rate;
  d.enemy_upgrade_at = c.enemy_upgrade_at;
  d.def_init_cost = c.defender_init_cost;
  d.atk_init_cost = c.attacker_init_cost;
  // integers within int32 by check_cfg (td_cfg_check.h): the conversions are exact
  d.frozen_time = (int32_t)c.frozen_time;
  d.base_LP = (int32_t)c.base_LP;
  d.tower_distance = (int32_t)c.tower_distance;
  d.atk_interval = (int32_t)c.attacker_action_interval;
  d.def_interval = (int32_t)c.defender_action_interval;
  d.max_episode_steps = c.max_episode_steps;
  d.max_cluster_length = c.max_cluster_length;
  d.max_tower_lv = c.max_tower_lv;
  d.upgrade_step = upgrade_step(d.max_episode_steps, d.enemy_upgrade_at);
}

// The checks themselves: td_cfg_check.h (run alone by scripts/cfg_check_host.cpp).
int check_cfg(const td_config& c) {
  char msg[200] = "";
  return cfg_check(c, msg, sizeof msg) == CFG_OK ? 0 : fail("%s", msg);
}

// Device allocations.  The library's own arrays are plain hipMalloc: every state array
// physically contiguous as well measured slower at most sizes (8,192 boards 35.1 vs 32.5
// us, 65,536 215.0 vs 210.4, profiles/r04/s25).  Callers' output buffers: td_alloc_device.
// *granted: whether the block is physically contiguous (a refused request falls back).
static hipError_t dev_malloc(void** p, size_t bytes, bool contiguous, bool* granted) {
  *granted = false;
  if (contiguous && hipExtMallocWithFlags(p, bytes, hipDeviceMallocContiguous) == hipSuccess) {
    *granted = true;
    return hipSuccess;
  }
  (void)hipGetLastError();  // (a refused contiguous request is not the caller's error)
  return hipMalloc(p, bytes);
}

// Live td_alloc_device blocks: how each was placed (td_alloc_is_contiguous) and its size.
struct Block { bool contiguous; size_t bytes; };
std::mutex g_blocks_mu;
std::unordered_map<const void*, Block> g_blocks;
// Live handles (td_free_device drops the retention of a buffer inside the freed block).
std::mutex g_handles_mu;
std::unordered_set<td_handle*> g_handles;

// The handle's device arrays, listed once: td_create allocates and zeroes them in this order,
// td_destroy frees them, and td_create's failure message sums them.  bytes = B * per_board + fixed.
struct DevArray {
  void** slot;
  size_t per_board, fixed;
};
#define TD_SLOT(m) reinterpret_cast<void**>(&h->m)
std::vector<DevArray> dev_arrays(td_handle* h) {
  const size_t w = sizeof(uint32_t);
  return {{TD_SLOT(d_cfg), 0, NCFG * sizeof(TdDevCfg)},
          {TD_SLOT(d_hdr), sizeof(TdHdr), 0},
          {TD_SLOT(d_en_lp), ECAP * sizeof(double), 0},
          {TD_SLOT(d_en_mg), ECAP * sizeof(double), 0},
          {TD_SLOT(d_en_inf), ECAP * w, 0},
          {TD_SLOT(d_tw_cd), TCAP * sizeof(double), 0},
          {TD_SLOT(d_tw_inf), TCAP * w, 0},
          {TD_SLOT(d_cells), (size_t)h->NC * w, 0},
          {TD_SLOT(d_opp), OPP_WORDS * w, 0},
          {TD_SLOT(d_hot), HOT_WORDS * w, 0},
          {TD_SLOT(d_np), OPP_WORDS * w, 0},
          {TD_SLOT(d_nxt), (size_t)NSLOT * slot_words(h->L) * w, 0},
          {TD_SLOT(d_lay_head), w, 0},
          {TD_SLOT(d_lay_tail), w, 0},
          {TD_SLOT(d_lay_claim), w, 0},
          {TD_SLOT(d_ovr_idx), sizeof(int32_t), 0},
          {TD_SLOT(d_scratch), h->scratch_stride, 0},
          {TD_SLOT(d_mask), 1, 0},
          {TD_SLOT(d_fail), 1, 0},
          {TD_SLOT(d_stage), 0, (size_t)h->stage_cap * h->lw * w},
          {TD_SLOT(d_epstats), 0, 2 * sizeof(double)},
          {TD_SLOT(d_lastep), sizeof(td_episode_record), 0},
          {TD_SLOT(d_guard_to), 0, w},
          {TD_SLOT(d_pairs), 2 * sizeof(int32_t), 0},
          {TD_SLOT(d_list_marks), w, 0},
          {TD_SLOT(d_list), 0, sizeof(ListState)}};
}
#undef TD_SLOT

int dalloc(void** p, size_t bytes) {
  HIP_OK(hipMalloc(p, std::max<size_t>(bytes, 1)));
  HIP_OK(hipMemset(*p, 0, std::max<size_t>(bytes, 1)));
  return 0;
}

StepArgs base_args(td_handle* h) {
  StepArgs a;
  std::memset(&a, 0, sizeof a);
  a.B = h->B; a.L = h->L; a.mode = h->mode; a.multi = h->multi; a.difficulty = h->difficulty;
  a.autoreset = h->autoreset;
  a.xcd_map = h->xcd_map;
  a.edge_wt = h->edge_wt;
  a.opp_np = h->opp_np;
  a.small = h->kernel.small;
  a.obs_wt = h->kernel.obs_wt;
  a.obs_f16 = h->obs_fmt == TD_OBS_F16 ? 1 : 0;
  a.frame_skip = h->frame_skip;
  a.hdr = h->d_hdr; a.en_lp = h->d_en_lp; a.en_mg = h->d_en_mg; a.en_inf = h->d_en_inf;
  a.tw_cd = h->d_tw_cd; a.tw_inf = h->d_tw_inf; a.cells = h->d_cells; a.opp_mt = h->d_opp; a.opp_hot = h->d_hot;
  a.np_mt = h->d_np; a.nxt = h->d_nxt; a.scratch = h->d_scratch; a.scratch_stride = h->scratch_stride;
  a.lay_head = h->d_lay_head; a.lay_tail = h->d_lay_tail; a.lay_claim = h->d_lay_claim;
  a.slot_words = slot_words(h->L);
  a.refill_grp = refill_group(h->B, h->refill_waves);
  a.refill_waves = h->refill_waves;
  a.refill_walks = kWalksPerStep * (h->refill_every > 0 ? h->refill_every : kRefillEvery);
  a.guard_to = h->d_guard_to;
  a.reset_fail = h->d_fail; a.cfg = h->d_cfg + h->epoch; a.cfgs = h->d_cfg; a.epoch = h->epoch;
  return a;
}

// fn(i) for i in [0, n) on a few host threads (seeding only).
template <class F>
void parallel_for(int n, F fn) {
  unsigned hw = std::thread::hardware_concurrency();
  int nt = std::max(1, std::min<int>((int)std::min(8u, hw ? hw : 1u), (n + 1023) / 1024));
  std::vector<std::thread> pool;
  for (int w = 0; w < nt; ++w)
    pool.emplace_back([&, w]() {
      for (int i = w; i < n; i += nt) fn(i);
    });
  for (auto& t : pool) t.join();
}

// MT19937 streams as the device keeps them: OPP_WORDS per board, the 624 words and the position,
// then the lazy boundary.  B of them, seeded by `seed` (np_seed, py_seed) from seeds[b].
std::vector<uint32_t> seeded_streams(size_t B, const uint32_t* seeds, void (*seed)(uint32_t*, uint32_t)) {
  std::vector<uint32_t> all(B * OPP_WORDS);
  parallel_for((int)B, [&](int b) {
    uint32_t* w = &all[(size_t)b * OPP_WORDS];
    seed(w, seeds[b]);
    w[MT_N + 1] = MT_N;  // no lazy words
  });
  return all;
}

// Board b's stream in the handle's array `arr` (d_opp, d_np) from or to a caller's 625 words,
// once the device is idle.  with_hot: position and lazy boundary live in the hot record.
int mt_put(td_handle* h, uint32_t* td_handle::*arr, int b, const uint32_t* mt) {
  if (!h || b < 0 || b >= h->B || !mt) return fail("bad board or NULL state");
  uint32_t w[OPP_WORDS];
  std::memcpy(w, mt, (MT_N + 1) * 4);
  w[MT_N + 1] = MT_N;  // no lazy words
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(h->*arr + (size_t)b * OPP_WORDS, w, sizeof w, hipMemcpyHostToDevice));
  return 0;
}
int mt_get(td_handle* h, uint32_t* td_handle::*arr, int b, uint32_t* mt, bool with_hot) {
  if (!h || b < 0 || b >= h->B || !mt) return fail("bad board or NULL state");
  uint32_t w[OPP_WORDS], hot[HOT_WORDS];
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(w, h->*arr + (size_t)b * OPP_WORDS, sizeof w, hipMemcpyDeviceToHost));
  if (with_hot) {
    HIP_OK(hipMemcpy(hot, h->d_hot + (size_t)b * HOT_WORDS, sizeof hot, hipMemcpyDeviceToHost));
    w[MT_N] = hot[0];
    w[MT_N + 1] = hot[1];
  }
  mt_finish_lazy(w);
  std::memcpy(mt, w, (MT_N + 1) * 4);
  return 0;
}

// Both step kernels of the handle (0 large, 1 small, 2 small2), resolved for its format and the
// boards resident in it (td_kernel_choice.h KernelChoice::resolve).
int apply_kernel(td_handle* h) {
  const int* r = h->resident[h->obs_fmt == TD_OBS_F16];
  // (while frame skip is on, td_step launches the skip kernel whatever kinds are kept here)
  // (for an aligned observation buffer: launch_step takes the large kernel for any other)
  h->kernel.resolve(h->L, h->mode, h->multi, h->obs_fmt, h->B, r[0], r[1]);
  return 0;
}

// A ring may have lost layouts, or the boards may consume them otherwise from here on: the ring
// guard runs before the next step, whatever its cadence.
void guard_next_step(td_handle* h) { h->since_guard = kGuardEvery; }

// Drop the staged layouts of boards [b0, b0 + count): they were drawn from a stream that has been replaced.
int drop_staged(td_handle* h, int b0, int count) {
  HIP_OK(hipDeviceSynchronize());
  guard_next_step(h);
  const size_t ring = (size_t)NSLOT * slot_words(h->L), n = (size_t)count;
  HIP_OK(hipMemset(h->d_nxt + (size_t)b0 * ring, 0, n * ring * 4));
  HIP_OK(hipMemset(h->d_lay_head + b0, 0, n * 4));
  HIP_OK(hipMemset(h->d_lay_tail + b0, 0, n * 4));
  HIP_OK(hipMemset(h->d_lay_claim + b0, 0, n * 4));
  // no pending draws (the RoadResume at the head of a board's scratch; the rest is a pending draw's alone)
  HIP_OK(hipMemset(h->d_scratch + (size_t)b0 * h->scratch_stride, 0, n * h->scratch_stride));
  return 0;
}

// Launch a ring refill behind the work queued on `s` so far, on the side streams in
// turn.  Refills are anchored to the step stream (each waits for the step before it,
// then runs beside the next one), never to host time: the host may run thousands of
// steps ahead of the GPU, and a refill launched "when a stream looks free" from there
// would leave the GPU without refills for as long.  A refill stuck on a draw the
// reference never finishes (milliseconds) delays only its own stream's queue.
// The refill is ordered after the work on s so far: after a reset kernel, whose
// draws-now use the boards' numpy streams and ring slots without a claim, and after the
// previous step (see kRefillEvery).
int start_refill(td_handle* h, hipStream_t s, bool after_step = false) {
  const int q = h->next_side;
  StepArgs a = base_args(h);
  hipEvent_t ev = after_step ? h->ev_step : h->ev_main;
  HIP_OK(hipEventRecord(ev, s));
  HIP_OK(hipStreamWaitEvent(h->side[q], ev, 0));
  HIP_OK(launch_refill(a, h->side[q]));
  h->next_side = (q + 1) % kSideStreams;
  return 0;
}

// The board mask of a reset or an opponent change on the device: the caller's B bytes, or every
// board where there are none.
int upload_mask(td_handle* h, const uint8_t* host_mask) {
  const std::vector<uint8_t> all(host_mask ? 0 : (size_t)h->B, 1);
  HIP_OK(hipMemcpy(h->d_mask, host_mask ? host_mask : all.data(), (size_t)h->B, hipMemcpyHostToDevice));
  return 0;
}

// What td_reset and td_reset_layouts share: the mask, a clean failure array and the reset kernel
// on s.  staged: the boards take the records in d_stage that d_ovr_idx names (td_reset_layouts).
int run_reset(td_handle* h, const uint8_t* host_mask, float* obs, bool staged, hipStream_t s) {
  if (upload_mask(h, host_mask)) return -1;
  HIP_OK(hipMemset(h->d_fail, 0, (size_t)h->B));
  StepArgs a = base_args(h);
  a.obs = obs;
  a.reset_mask = h->d_mask;
  a.ovr_idx = staged ? h->d_ovr_idx : nullptr;
  a.ovr_rec = staged ? h->d_stage : nullptr;
  HIP_OK(launch_reset(a, s));
  guard_next_step(h);  // a reset consumed layouts: guard before the next step
  return 0;
}

// td_kernel_timing: the event pair of the next timed dispatch, or none once tev_cap are out.
// The list calls (copies and partial steps) take one whatever `every` is; td_step asks at its
// cadence (at_cadence: none between two timed steps).
struct EvPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
};
EvPair next_timing_pair(td_handle* h, bool at_cadence = false) {
  EvPair p;
  if (at_cadence && (h->steps - h->tev_from) % h->tev_every != 0) return p;
  if (h->tev_n < h->tev_cap) {
    p.e0 = h->tev[2 * (size_t)h->tev_n];
    p.e1 = h->tev[2 * (size_t)h->tev_n + 1];
    h->tev_n += 1;
  }
  return p;
}

// The caller's ids to d_pairs on the call's stream, through the next pinned slot, so the
// caller's arrays are free on return: ids0[0 .. n), then ids1[0 .. n) where given.
int upload_ids(td_handle* h, const int32_t* ids0, const int32_t* ids1, int n, hipStream_t s) {
  const int q = h->id_next;
  // (an event never recorded is complete; else this waits for the upload kIdSlots calls ago only)
  HIP_OK(hipEventSynchronize(h->id_ev[q]));
  int32_t* stage = h->id_stage + (size_t)q * 2 * (size_t)h->B;
  const size_t bytes = (size_t)n * sizeof(int32_t);
  std::memcpy(stage, ids0, bytes);
  if (ids1) std::memcpy(stage + n, ids1, bytes);
  HIP_OK(hipMemcpyAsync(h->d_pairs, stage, ids1 ? 2 * bytes : bytes, hipMemcpyHostToDevice, s));
  HIP_OK(hipEventRecord(h->id_ev[q], s));
  h->id_next = (q + 1) % kIdSlots;
  return 0;
}

// The check of a device-resident list on the call's stream, in front of the kernel that
// consumes it (td_list_check.hip): src == nullptr for a step's list.  The call takes the next
// serial; its epoch stamps the marks, so the scratch is cleared only once per round of epochs.
int enqueue_list_check(td_handle* h, const int32_t* src, const int32_t* dst, int cap, const int32_t* count,
                       td_list_status* status, hipStream_t s) {
  ListCheckArgs c{};
  c.src = src; c.dst = dst; c.count = count; c.cap = cap; c.B = h->B;
  c.call = (int)(h->list_calls & 0x7fffffff);
  c.epoch = list_epoch(h->list_calls);
  c.marks = h->d_list_marks; c.st = h->d_list; c.status = status;
  if (c.epoch == 1 && h->list_calls != 0) HIP_OK(hipMemsetAsync(h->d_list_marks, 0, (size_t)h->B * sizeof(uint32_t), s));
  HIP_OK(launch_list_check(c, s));
  h->list_calls += 1;
  return 0;
}

// A device list's cap and pointers against B boards (td_call_check.h list_args_check): 1 go on,
// 0 an empty list (the call returns 0), -1 refused.  B = 0 where a call has no handle yet: cap < 0.
int check_list_args(const char* fn, int cap, int B, bool have_lists, const char* lists) {
  char msg[200];
  const int go = list_args_check(fn, cap, B, have_lists, lists, msg, sizeof msg);
  return go == LIST_ARGS_REFUSED ? fail("%s", msg) : go;
}

// cap < 0 needs no handle: a device-list call with an io refuses it once the io's two header
// words match, in front of the handle's checks.  True: refused.
template <class Io>
bool negative_cap_refused(const char* fn, const Io* io, int cap) {
  return io && io->size == (uint32_t)sizeof(Io) && io->abi == (uint32_t)TD_ABI_VERSION && cap < 0 &&
         check_list_args(fn, cap, 0, false, "") < 0;
}

// What the mask and sample kernels read of the handle's boards.
BoardView board_view(const td_handle* h) {
  return {h->B, h->L, h->multi, h->xcd_map, h->d_hdr, h->d_tw_inf, h->d_cells, h->d_cfg + h->epoch};
}

// The list forms of the calls that take an io and serve a list with one kernel family (the masks,
// the sampler, the playouts), each written once over the call's io check and its list kernel's
// launch.  The masks and the sampler only read state: no launches for the refill cadence or the
// ring guard, no timing pair, the observation ledger left alone; a playout's launch function
// brackets its kernel as a partial step's (launch_playout_call).
// H: `const td_handle` for the calls that only read state, `td_handle` for a call whose launch counts
// in the handle (the playouts).
template <class Io, class Args, class H = const td_handle>
using IoCheck = int (*)(const char* fn, H* h, const Io* io, Args* out);
template <class Args>
using ListLaunch = hipError_t (*)(const Args& a, const int32_t* ids, int cap, const int32_t* count,
                                  const td_list_status* verdict, hipStream_t s);
// What a call puts on the stream in front of its ids or its list check (the playouts: the refill
// and the ring guard, where td_step_boards[_dev] put them); nullptr: nothing.
template <class Args>
using ListBefore = int (*)(const Args& a, hipStream_t s);

// A host list.  Everything is checked here, before anything is enqueued; the ids reach the kernel
// through the pinned id slots and d_pairs (upload_ids), as td_step_boards'.
template <class Io, class Args, class H>
int read_boards(const char* fn, IoCheck<Io, Args, H> check, ListLaunch<Args> launch, td_handle* h, const Io* io,
                const int32_t* boards, int n, void* stream, ListBefore<Args> before = nullptr) {
  Args a;
  if (check(fn, h, io, &a)) return -1;
  char msg[200];
  if (ids_check(boards, n, h->B, h->id_role, msg, sizeof msg) != IDS_OK) return fail("%s: %s", fn, msg);
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (before && before(a, s)) return -1;
  if (upload_ids(h, boards, nullptr, n, s)) return -1;
  HIP_OK(launch(a, h->d_pairs, n, nullptr, nullptr, s));
  return 0;
}

// A list, its length and its verdict in device memory, under td_step_boards_dev's contract: the
// host checks what it can see, the check kernel the contents, on the stream in front of the list
// kernel (the call takes the next serial); a refused list writes no output byte.
template <class Io, class Args, class H>
int read_boards_dev(const char* fn, IoCheck<Io, Args, H> check, ListLaunch<Args> launch, td_handle* h, const Io* io,
                    const int32_t* boards_dev, int cap, const int32_t* count_dev, td_list_status* status_dev,
                    void* stream, ListBefore<Args> before = nullptr) {
  if (negative_cap_refused(fn, io, cap)) return -1;
  Args a;
  if (check(fn, h, io, &a)) return -1;
  if (const int go = check_list_args(fn, cap, h->B, boards_dev, "boards_dev"); go <= 0) return go;
  hipStream_t s = (hipStream_t)stream;
  if (before && before(a, s)) return -1;
  if (enqueue_list_check(h, nullptr, boards_dev, cap, count_dev, status_dev, s)) return -1;
  HIP_OK(launch(a, boards_dev, cap, count_dev, &h->d_list->verdict, s));
  return 0;
}

// td_create's memory: the device arrays, zeroed, and the pinned id slots with their events.
int create_memory(td_handle* h) {
  const size_t B = (size_t)h->B;
  for (const DevArray& a : dev_arrays(h))
    if (dalloc(a.slot, B * a.per_board + a.fixed)) return -1;
  if (hipHostMalloc((void**)&h->id_stage, kIdSlots * 2 * B * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
    return fail("td_create: %zu B of pinned host memory (td_copy_boards' index slots)", kIdSlots * 2 * B * sizeof(int32_t));
  for (int q = 0; q < kIdSlots; ++q) HIP_OK(hipEventCreateWithFlags(&h->id_ev[q], hipEventDisableTiming));
  return 0;
}

// Everything td_create sets up once the handle's ints are in place, in order; returns at the
// first failure with its message (td_destroy then frees what there is).
int create_setup(td_handle* h) {
  const size_t B = (size_t)h->B;
  if (create_memory(h)) {  // name the footprint (the staged-layout rings are most of it at large L)
    const double ring = (double)B * NSLOT * slot_words(h->L) * 4.0;
    double total = 0.0;  // everything asked for, the rings included
    for (const DevArray& a : dev_arrays(h)) total += (double)(B * a.per_board + a.fixed);
    std::string e = g_err;
    return fail("td_create: %d boards at L = %d need %.1f MB of device memory (%.1f MB of it the staged-layout rings, "
                "%d x %d words per board): %s", h->B, h->L, total / 1e6, ring / 1e6, NSLOT, slot_words(h->L), e.c_str());
  }
  {  // win = -1: no finished episode yet
    std::vector<td_episode_record> init((size_t)B, td_episode_record{0.0, 0, -1});
    HIP_OK(hipMemcpy(h->d_lastep, init.data(), B * sizeof(td_episode_record), hipMemcpyHostToDevice));
  }
  HIP_OK(hipMemcpy(h->d_cfg, &h->dcfg, sizeof(TdDevCfg), hipMemcpyHostToDevice));
  {  // no defect pending; the marks are zero: no epoch (>= 1) has marked a board
    ListState ls{};
    ls.key = kListNoDefect;
    HIP_OK(hipMemcpy(h->d_list, &ls, sizeof ls, hipMemcpyHostToDevice));
  }
  for (int q = 0; q < kSideStreams; ++q)  // side streams (layout refills)
    HIP_OK(hipStreamCreateWithFlags(&h->side[q], hipStreamNonBlocking));
  HIP_OK(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
  // The step-cadence refill needs the previous step finished, not its memory fenced:
  // everything a refill reads of a step (lay_head) and publishes (slots, tags, claims,
  // the stream) goes through write-through / atomic accesses.  Without the event's
  // system-scope fence (a cache writeback): -0.6 % / -0.8 % per step at 8,192 / 4,096
  // boards (profiles/r03/s17).
  HIP_OK(hipEventCreateWithFlags(&h->ev_step, hipEventDisableTiming | hipEventDisableSystemFence));
  {  // boards resident at once, per format and kernel: what TD_KERNEL_AUTO goes by (auto_kernel)
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
    StepArgs ra = base_args(h);
    for (int f = 0; f < 2; ++f) {
      ra.obs_f16 = f;
      h->resident[f][0] = step_resident_boards(ra, cus, 1);
      h->resident[f][1] = step_resident_boards(ra, cus, 2);
    }
    if (apply_kernel(h)) return -1;
  }
  std::vector<uint32_t> seeds(B);
  for (size_t b = 0; b < B; ++b) seeds[b] = (uint32_t)b;
  return td_seed(h, seeds.data(), seeds.data());
}

// td_step_io_init, td_mask_io_init, td_sample_io_init, td_sample_w_io_init: all zero but the two header words.
template <class IO>
void io_init(IO* io) {
  if (!io) return;
  std::memset(io, 0, sizeof *io);
  io->size = (uint32_t)sizeof(IO);
  io->abi = TD_ABI_VERSION;
}

// td_create gives up: the handle goes, the message stays.
td_handle* create_failed(td_handle* h) {
  std::string e = g_err;
  td_destroy(h);
  g_err = e;
  return nullptr;
}

}  // namespace

extern "C" {

int td_abi_version(void) { return TD_ABI_VERSION; }

int td_step_io_size(void) { return (int)sizeof(td_step_io); }

int td_alloc_device(size_t bytes, int device, int contiguous, void** out) {
  if (!out || bytes == 0) return fail("td_alloc_device: bad arguments");
  *out = nullptr;
  int prev = 0;
  HIP_OK(hipGetDevice(&prev));
  HIP_OK(hipSetDevice(device));
  bool granted = false;
  hipError_t e = dev_malloc(out, bytes, contiguous != 0, &granted);
  if (e == hipSuccess) e = hipMemset(*out, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // zeroed before any stream uses it
  (void)hipSetDevice(prev);  // (the caller's current device is left as it was)
  if (e != hipSuccess) {
    if (*out) (void)hipFree(*out);
    *out = nullptr;
    return fail("td_alloc_device: %s", hipGetErrorString(e));
  }
  std::lock_guard<std::mutex> g(g_blocks_mu);
  g_blocks[*out] = Block{granted, bytes};
  return 0;
}

int td_free_device(void* p) {
  if (!p) return 0;
  size_t bytes = 0;
  {
    std::lock_guard<std::mutex> g(g_blocks_mu);
    auto it = g_blocks.find(p);
    if (it != g_blocks.end()) {
      bytes = it->second.bytes;
      g_blocks.erase(it);
    }
  }
  {  // a later allocation may reuse the address: no handle may take it for the buffer it retained
    std::lock_guard<std::mutex> g(g_handles_mu);
    for (td_handle* h : g_handles) h->ledger.freed(p, bytes);
  }
  HIP_OK(hipFree(p));
  return 0;
}

int td_alloc_is_contiguous(const void* p) {
  std::lock_guard<std::mutex> g(g_blocks_mu);
  auto it = g_blocks.find(p);
  return it == g_blocks.end() ? -1 : it->second.contiguous ? 1 : 0;
}

void td_step_io_init(td_step_io* io) { io_init(io); }

const char* td_last_error(void) { return g_err.c_str(); }

void td_config_default(td_config* c) {
  // gym_TD/envs/TDParam.py:2-64, :105-111
  std::memset(c, 0, sizeof *c);
  const double lp[4][2] = {{820, 1700}, {2050, 3000}, {6000, 8000}, {8000, 12000}};
  const double sp[4][2] = {{.25, .25}, {.13, .13}, {.1, .1}, {.1, .1}};
  const double df[4][2] = {{0, 0}, {200, 250}, {600, 800}, {80, 100}};
  const double ec[4][2] = {{8, 8}, {15, 15}, {40, 40}, {30, 30}};
  const double ta[4][2] = {{454, 540}, {651, 771}, {566, 691}, {358, 424}};
  const double tr[4][2] = {{3, 3}, {2, 2}, {4, 4}, {3, 3}};
  const double ts[4][2] = {{0, 0}, {0, 0}, {1, 1}, {0, 0}};
  const double tc[4][2] = {{10, 10}, {17, 17}, {23, 23}, {12, 12}};
  const double ti[4][2] = {{2, 2}, {4, 4}, {7, 7}, {4.75, 4.75}};
  std::memcpy(c->enemy_LP, lp, sizeof lp);
  std::memcpy(c->enemy_speed, sp, sizeof sp);
  std::memcpy(c->enemy_defense, df, sizeof df);
  std::memcpy(c->enemy_cost, ec, sizeof ec);
  std::memcpy(c->tower_attack, ta, sizeof ta);
  std::memcpy(c->tower_range, tr, sizeof tr);
  std::memcpy(c->tower_splash_range, ts, sizeof ts);
  std::memcpy(c->tower_cost, tc, sizeof tc);
  std::memcpy(c->tower_attack_interval, ti, sizeof ti);
  c->tower_destruct_return = .5;
  c->frozen_time = 2;
  c->frozen_ratio = .2;
  c->attacker_init_cost = 0;
  c->defender_init_cost = 10;
  c->base_LP = 5;
  c->max_cost = 100;
  c->reward_kill = 0.1;
  c->penalty_leak = 10.;
  c->reward_time = 0.001;
  c->attacker_cost_init_rate = .5;
  c->attacker_cost_final_rate = 1;
  c->defender_cost_rate = .2;
  c->tower_distance = 2;
  c->enemy_upgrade_at = 0.75;
  c->attacker_action_interval = 1;
  c->defender_action_interval = 1;
  c->max_enemy_lv = 1;
  c->max_tower_lv = 1;
  c->enemy_types = 4;
  c->tower_types = 4;
  c->max_episode_steps = 1200;
  c->max_cluster_length = 8;
  c->max_num_of_roads = 3;
}

td_handle* td_create(const td_config* cfg, int map_size, int n_boards, int mode, int multi_action, int difficulty,
                     int device) {
  if (!cfg) { fail("td_create: cfg is NULL"); return nullptr; }
  if (check_cfg(*cfg)) return nullptr;
  if (map_size < 4 || map_size > 32) { fail("map_size must be in [4, 32], got %d", map_size); return nullptr; }
  if (n_boards < 1) { fail("n_boards must be >= 1"); return nullptr; }
  if (mode < 0 || mode > 2) { fail("mode must be 0 (def), 1 (atk) or 2 (2p)"); return nullptr; }
  if (mode == TD_MODE_DEF && (difficulty < 0 || difficulty > 1)) { fail("TD-def difficulty must be 0 or 1 (random_enemy_lv0/lv1)"); return nullptr; }
  if (mode == TD_MODE_ATK && (difficulty < 0 || difficulty > 2)) { fail("TD-atk difficulty must be 0, 1 or 2 (random_tower_lv0/1/2)"); return nullptr; }
  if (mode == TD_MODE_ATK && multi_action) { fail("TD-atk has no multi-action defender"); return nullptr; }
  if (hipSetDevice(device) != hipSuccess) {
    fail("hipSetDevice(%d) failed: %s", device, hipGetErrorString(hipGetLastError()));
    return nullptr;
  }
  td_handle* h = new td_handle();
  h->L = map_size; h->NC = map_size * map_size; h->B = n_boards; h->mode = mode; h->multi = multi_action ? 1 : 0;
  h->difficulty = difficulty; h->device = device; h->lw = layout_words(map_size);
  h->ledger.B = n_boards;
  h->scratch_stride = (sizeof(RoadResume) + road_scratch_bytes(map_size) + 15) & ~(size_t)15;
  h->stage_cap = std::min(n_boards, 4096);
  build_dev_cfg(*cfg, h->dcfg);
  if (create_setup(h)) return create_failed(h);
  {
    std::lock_guard<std::mutex> g(g_handles_mu);
    g_handles.insert(h);
  }
  return h;
}

void td_destroy(td_handle* h) {
  if (!h) return;
  {
    std::lock_guard<std::mutex> g(g_handles_mu);
    g_handles.erase(h);
  }
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (const DevArray& a : dev_arrays(h))
    if (*a.slot) (void)hipFree(*a.slot);
  if (h->id_stage) (void)hipHostFree(h->id_stage);
  for (hipEvent_t e : h->id_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->ev_main) (void)hipEventDestroy(h->ev_main);
  if (h->ev_step) (void)hipEventDestroy(h->ev_step);
  for (hipEvent_t e : h->tev) (void)hipEventDestroy(e);
  for (int q = 0; q < kSideStreams; ++q)
    if (h->side[q]) (void)hipStreamDestroy(h->side[q]);
  delete h;
}

// paramConfig on a live engine (TDParam.py:98-100).  The reference reads most values
// live from `config`, but an Enemy / Tower keeps the stats it was created (or upgraded)
// with and a TDBoard the max_cost / base_LP of its reset.  So a new block becomes the
// current epoch; entities keep referring to the block of their own epoch.  Blocks are
// recycled only when no live enemy or tower refers to them (td_cfg_usage_kernel).
int td_set_config(td_handle* h, const td_config* cfg) {
  if (!h || !cfg) return fail("td_set_config: NULL argument");
  if (check_cfg(*cfg)) return -1;
  TdDevCfg d;
  build_dev_cfg(*cfg, d);
  HIP_OK(hipDeviceSynchronize());
  if (std::memcmp(&d, &h->dcfg, sizeof d) == 0) return 0;  // nothing changed
  // tower_distance may not grow while a board holds a tower.  The reference subtracts a destructed
  // tower's diamond at the CURRENT tower_distance (TDBoard.py:281-287): wider than the one it added,
  // it takes map[6] below zero on cells it never counted, and to zero under another tower -- a free
  // cell, so a second tower can stand on a cell that has one.  A cell word has an unsigned count and
  // room for one tower: neither state can be represented, so the change that leads there is refused.
  if (d.tower_distance > h->dcfg.tower_distance) {
    std::vector<TdHdr> hdr((size_t)h->B);
    HIP_OK(hipMemcpy(hdr.data(), h->d_hdr, hdr.size() * sizeof(TdHdr), hipMemcpyDeviceToHost));
    for (int b = 0; b < h->B; ++b)
      if (hdr[(size_t)b].n_tw > 0)
        return fail("td_set_config: tower_distance may not grow (%d -> %d) while a board holds a tower (board %d has %d): "
                    "reset the boards, or destruct the towers, first",
                    h->dcfg.tower_distance, d.tower_distance, b, hdr[(size_t)b].n_tw);
  }
  int slot = -1;
  if (h->cfg_fresh < NCFG) {
    slot = h->cfg_fresh++;
  } else {
    uint32_t* d_used = nullptr;
    HIP_OK(hipMalloc((void**)&d_used, NCFG / 8));
    HIP_OK(hipMemset(d_used, 0, NCFG / 8));
    StepArgs a = base_args(h);
    const hipError_t e = launch_cfg_usage(a, d_used, nullptr);
    uint32_t used[NCFG / 32];
    const hipError_t e2 = e == hipSuccess ? hipMemcpy(used, d_used, sizeof used, hipMemcpyDeviceToHost) : e;
    (void)hipFree(d_used);
    HIP_OK(e2);
    for (int k = 0; k < NCFG && slot < 0; ++k)
      if (k != h->epoch && !((used[k / 32] >> (k % 32)) & 1u)) slot = k;
    if (slot < 0) return fail("td_set_config: %d configs are still referenced by live enemies/towers", NCFG);
  }
  HIP_OK(hipMemcpy(h->d_cfg + slot, &d, sizeof d, hipMemcpyHostToDevice));
  h->dcfg = d;
  h->epoch = slot;
  h->ledger.touch();  // channels 21-24 and 41-44 read the current block
  return 0;
}

// Both mode setters first wait for the device: a refill may still be drawing on a side
// stream.  Layouts staged so far stay valid for random_agent=True (they are the stream's
// next layouts, in order), so turning auto-reset off keeps them for explicit resets.
int td_config_epoch(td_handle* h) { return h ? h->epoch : fail("NULL handle"); }

int td_set_autoreset(td_handle* h, int on) {
  if (!h) return fail("NULL handle");
  HIP_OK(hipDeviceSynchronize());
  h->autoreset = on ? 1 : 0;
  guard_next_step(h);
  return 0;
}

// random_agent=False interleaves the opponent's draws with the layout draws on one
// stream, so no layout may have been drawn ahead of play: refused while any board has a
// staged layout or a pending draw (td_seed with new numpy seeds, or running the staged
// layouts out with explicit resets, clears them).
int td_set_random_agent(td_handle* h, int random_agent) {
  if (!h) return fail("NULL handle");
  if (!random_agent && h->frame_skip > 1)
    return fail("random_agent=False: not supported with frame skip (td_frame_skip() = %d); set td_set_frame_skip(h, 1) first",
                h->frame_skip);
  HIP_OK(hipDeviceSynchronize());
  guard_next_step(h);
  if (!random_agent && !h->opp_np) {
    std::vector<uint32_t> head((size_t)h->B), tail((size_t)h->B);
    HIP_OK(hipMemcpy(head.data(), h->d_lay_head, (size_t)h->B * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tail.data(), h->d_lay_tail, (size_t)h->B * 4, hipMemcpyDeviceToHost));
    std::vector<RoadResume> res((size_t)h->B);
    HIP_OK(hipMemcpy2D(res.data(), sizeof(RoadResume), h->d_scratch, h->scratch_stride, sizeof(RoadResume),
                       (size_t)h->B, hipMemcpyDeviceToHost));
    for (int b = 0; b < h->B; ++b)
      if (head[(size_t)b] != tail[(size_t)b] || res[(size_t)b].phase != RP_NEW)
        return fail("random_agent=False: board %d has layouts drawn ahead of play (auto-reset refills); "
                    "set it before the first reset, or re-seed the layout streams first", b);
  }
  h->opp_np = random_agent ? 0 : 1;
  return 0;
}

int td_seed(td_handle* h, const uint32_t* np_seeds, const uint32_t* py_seeds) {
  if (!h) return fail("NULL handle");
  const size_t B = (size_t)h->B;
  if (np_seeds) {
    const std::vector<uint32_t> nw = seeded_streams(B, np_seeds, np_seed);
    if (drop_staged(h, 0, h->B)) return -1;
    HIP_OK(hipMemcpy(h->d_np, nw.data(), B * OPP_WORDS * 4, hipMemcpyHostToDevice));
  }
  if (py_seeds) {
    const std::vector<uint32_t> op = seeded_streams(B, py_seeds, py_seed);
    std::vector<uint32_t> hot(B * HOT_WORDS, 0u);
    for (size_t b = 0; b < B; ++b) { hot[b * HOT_WORDS] = MT_N; hot[b * HOT_WORDS + 1] = MT_N; }
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h->d_opp, op.data(), B * OPP_WORDS * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(h->d_hot, hot.data(), B * HOT_WORDS * 4, hipMemcpyHostToDevice));
  }
  return 0;
}

int td_set_py_state(td_handle* h, int b, const uint32_t* mt) {
  if (mt_put(h, &td_handle::d_opp, b, mt)) return -1;
  const uint32_t hot[HOT_WORDS] = {mt[MT_N], MT_N, 0u};
  HIP_OK(hipMemcpy(h->d_hot + (size_t)b * HOT_WORDS, hot, sizeof hot, hipMemcpyHostToDevice));
  return 0;
}
// The device keeps the opponent's position in the hot record and may have
// pre-drawn (and lazily twisted) ahead of it; the exported state is CPython's
// getstate() form of the same stream (equal future draws).
int td_get_py_state(td_handle* h, int b, uint32_t* mt) { return mt_get(h, &td_handle::d_opp, b, mt, true); }
int td_get_np_state(td_handle* h, int b, uint32_t* mt) { return mt_get(h, &td_handle::d_np, b, mt, false); }
int td_set_np_state(td_handle* h, int b, const uint32_t* mt) {
  return mt_put(h, &td_handle::d_np, b, mt) ? -1 : drop_staged(h, b, 1);
}

int td_reset(td_handle* h, const uint8_t* host_mask, float* obs, void* stream) {
  if (!h) return fail("NULL handle");
  hipStream_t s = (hipStream_t)stream;
  HIP_OK(hipDeviceSynchronize());
  const bool mine = h->ledger.reset_into(obs);
  ObsLedger::Guard guard{&h->ledger};
  if (run_reset(h, host_mask, obs, false, s)) return -1;
  if (h->autoreset && !h->opp_np && start_refill(h, s)) return -1;
  HIP_OK(hipDeviceSynchronize());
  std::vector<uint8_t> fl((size_t)h->B);
  HIP_OK(hipMemcpy(fl.data(), h->d_fail, (size_t)h->B, hipMemcpyDeviceToHost));
  h->last_reset_failed.clear();
  for (int b = 0; b < h->B; ++b) {
    if (host_mask && !host_mask[(size_t)b]) continue;
    if (fl[(size_t)b]) h->last_reset_failed.push_back(b);
    else if (mine) h->ledger.mark(b);  // (a board whose draw failed keeps its state, and its observation)
  }
  guard.ok = true;
  return (int)h->last_reset_failed.size();
}

int td_last_reset_failures(td_handle* h, int32_t* boards, int cap) {
  if (!h) return fail("NULL handle");
  int n = (int)h->last_reset_failed.size();
  for (int i = 0; i < n && i < cap && boards; ++i) boards[i] = h->last_reset_failed[(size_t)i];
  return n;
}

int td_reset_layouts(td_handle* h, const uint32_t* recs, const int32_t* boards, int n, float* obs, void* stream) {
  if (!h || (n > 0 && (!recs || !boards))) return fail("td_reset_layouts: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n; ++i)
    if (boards[i] < 0 || boards[i] >= h->B || recs[(size_t)i * h->lw] != TD_LAYOUT_MAGIC)
      return fail("td_reset_layouts: bad board id or layout record %d", i);
  // the step kernels take num_roads and max dist on trust: the channel-9 table has
  // MAX_ROAD_CELLS entries, indexed by a cell's distance <= max dist
  for (int i = 0; i < n; ++i) {
    const uint32_t* r = recs + (size_t)i * h->lw;
    if (r[1] < 1 || r[1] > 3 || r[3] > (uint32_t)(MAX_ROAD_CELLS - 1))
      return fail("td_reset_layouts: layout record %d has num_roads %u / max dist %u (must be 1..3 / 0..%d: "
                  "a road has at most %d cells)", i, r[1], r[3], MAX_ROAD_CELLS - 1, MAX_ROAD_CELLS);
  }
  HIP_OK(hipDeviceSynchronize());
  const bool mine = n > 0 && h->ledger.reset_into(obs);
  ObsLedger::Guard guard{&h->ledger};
  std::vector<int32_t> idx((size_t)h->B, -1);
  for (int i0 = 0; i0 < n; i0 += h->stage_cap) {
    const int m = std::min(h->stage_cap, n - i0);
    std::vector<uint8_t> mask((size_t)h->B, 0);
    std::fill(idx.begin(), idx.end(), -1);
    for (int i = 0; i < m; ++i) { idx[(size_t)boards[i0 + i]] = i; mask[(size_t)boards[i0 + i]] = 1; }
    HIP_OK(hipMemcpy(h->d_stage, recs + (size_t)i0 * h->lw, (size_t)m * h->lw * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(h->d_ovr_idx, idx.data(), (size_t)h->B * 4, hipMemcpyHostToDevice));
    if (run_reset(h, mask.data(), obs, true, s)) return -1;
    HIP_OK(hipStreamSynchronize(s));
    for (int i = 0; mine && i < m; ++i) h->ledger.mark(boards[i0 + i]);
  }
  guard.ok = true;
  return 0;
}

// Boards dst[i] become copies of boards src[i] on the device (td_copy.hip), asynchronously on
// the step's stream.  The ids are checked here, before anything is enqueued; they reach the
// kernel through a pinned slot and d_pairs, so the caller's arrays are free on return.
int td_copy_boards(td_handle* h, const int32_t* src, const int32_t* dst, int n, float* obs, void* stream) {
  if (!h) return fail("td_copy_boards: NULL handle");
  char msg[200];
  if (copy_check(src, dst, n, h->B, h->id_role, msg, sizeof msg) != COPY_OK) return fail("td_copy_boards: %s", msg);
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  // the destinations' states change: rows written into the retained buffer keep it current,
  // any other buffer (or none) leaves it behind
  const bool mine = h->ledger.reset_into(obs);
  ObsLedger::Guard guard{&h->ledger};
  if (upload_ids(h, src, dst, n, s)) return -1;
  StepArgs a = base_args(h);
  a.obs = obs;
  const EvPair ev = next_timing_pair(h);  // a copy kernel's dispatch is timed too, whatever `every` is
  HIP_OK(launch_copy(a, h->d_pairs, n, s, ev.e0, ev.e1));
  for (int i = 0; mine && i < n; ++i) h->ledger.mark(dst[i]);  // (a destination without an episode is written whole by its next step)
  guard.ok = true;
  return 0;
}

namespace {

// What td_step and td_step_boards check of their io before anything else, and the step
// arguments they make of it.  fn: the caller's name, for the message.
int check_step_io(const char* fn, const td_handle* h, const td_step_io* io) {
  if (!io) return fail("%s: NULL io", fn);
  // The two header words first (every td_step_io of any ABI has >= 8 bytes): a caller
  // built against another layout is refused before any pointer of its struct is read.
  if (io->size != (uint32_t)sizeof(td_step_io) || io->abi != (uint32_t)TD_ABI_VERSION)
    return fail("%s: td_step_io has size %u / abi %u, this library expects size %u / abi %d "
                "(set io.size = sizeof(td_step_io) and io.abi = TD_ABI_VERSION, or call td_step_io_init; "
                "an ABI-2 struct has no header)",
                fn, io->size, io->abi, (unsigned)sizeof(td_step_io), TD_ABI_VERSION);
  if (!h) return fail("%s: NULL handle", fn);
  if (!io->obs || !io->reward || !io->done) return fail("%s: obs, reward and done are required", fn);
  if (h->mode != TD_MODE_ATK && !io->def_act) return fail("%s: def_act required in this mode", fn);
  if (h->mode != TD_MODE_DEF && !io->atk_act) return fail("%s: atk_act required in this mode", fn);
  return 0;
}

StepArgs step_args(td_handle* h, const td_step_io* io) {
  StepArgs a = base_args(h);
  a.def_act = io->def_act; a.atk_act = io->atk_act; a.obs = io->obs; a.reward = io->reward; a.done = io->done;
  a.real_def = io->real_def; a.real_atk = io->real_atk; a.fail_def = io->fail_def; a.fail_atk = io->fail_atk;
  a.win = io->win; a.allow_next = io->allow_next; a.ep_return = io->ep_return; a.ep_len = io->ep_len;
  a.cooldowns = io->cooldowns;
  a.ep_stats = h->d_epstats;
  a.last_ep = h->d_lastep;
  return a;
}

// What goes in front of a step launch on its stream: the side refill at its cadence and the
// ring guard (kGuardEvery).  Both count launches: a board consumes at most one staged layout
// per launch, whether the launch steps every board or some.
int before_step_launch(td_handle* h, const StepArgs& a, hipStream_t s) {
  // the refill goes first: it waits for the previous step only, so a board whose ring
  // is dry in this step can wait for it (td_step_body.h step_board) without a cycle
  // random_agent=True: layouts are staged ahead by refills on the side streams.
  // random_agent=False: they are drawn in stream order right after the step (td_step).
  if (h->autoreset && !h->opp_np && h->refill_every > 0 && (h->steps % h->refill_every) == 0 &&
      start_refill(h, s, true))
    return -1;
  // the ring guard: behind the previous step, beside the refill just launched
  if (h->autoreset && !h->opp_np && h->guard_every > 0 && h->since_guard >= h->guard_every) {
    HIP_OK(launch_refill(a, s, h->guard_every));
    h->since_guard = 0;
  }
  return 0;
}

// What a stepping launch leaves behind, whether it stepped every board or some: one more launch
// for the refill cadence and td_kernel_timing's, one more since the ring guard.
void step_launched(td_handle* h) {
  h->steps += 1;
  h->since_guard += 1;
}

// check_step_io, then what a partial step asks of the handle's settings (td_call_check.h).
int check_partial_step(const char* fn, const td_handle* h, const td_step_io* io) {
  if (check_step_io(fn, h, io)) return -1;
  char msg[240];
  return partial_step_refused(fn, h->frame_skip, h->opp_np, h->autoreset, msg, sizeof msg) ? fail("%s", msg) : 0;
}

}  // namespace

int td_step(td_handle* h, const td_step_io* io, void* stream) {
  if (check_step_io("td_step", h, io)) return -1;
  hipStream_t s = (hipStream_t)stream;
  StepArgs a = step_args(h, io);
  // td_retain_obs: a step into the retained buffer may skip what the buffer already holds;
  // any other step writes every byte and leaves the retained buffer behind.
  const bool retained = h->ledger.is_retained(io->obs);
  a.obs_skip = h->ledger.full_step_skips(io->obs) ? 1 : 0;
  ObsLedger::Guard guard{&h->ledger};
  if (before_step_launch(h, a, s)) return -1;
  const EvPair ev = next_timing_pair(h, true);
  // frame skip: one launch of the skip kernel runs the k board steps (td_step_skip.h).  The refill
  // cadence and the ring guard above count launches: a board consumes at most one layout per launch.
  if (h->frame_skip > 1) {
    HIP_OK(launch_skip(a, s, ev.e0, ev.e1));
  } else {
    // the kernel is chosen per launch: a launch that writes every window is bound by its stores,
    // a skipping launch by the boards in flight (td_kernel_choice.h retained_kernel_kind)
    a.small = h->kernel.kind(a.obs_skip);
    a.obs_wt = h->kernel.write_through(a.obs_skip);
    HIP_OK(launch_step(a, a.small, s, ev.e0, ev.e1));
    h->kernel.name_kind = step_launch_kind(a, a.small);
  }
  if (h->autoreset && h->opp_np) HIP_OK(launch_autoreset(a, s));
  step_launched(h);
  if (!retained) h->ledger.touch();
  else if (!a.obs_skip) h->ledger.mark_all();  // every board's observation is in the retained buffer now
  guard.ok = true;
  return 0;
}

// One env step for the boards named, every other board left as it is (td_step_sel.hip),
// asynchronously on the step's stream.  Everything is checked here, before anything is enqueued;
// the ids reach the kernel through the pinned id slots and d_pairs (upload_ids), so the caller's
// array is free on return.
int td_step_boards(td_handle* h, const td_step_io* io, const int32_t* boards, int n, void* stream) {
  if (check_partial_step("td_step_boards", h, io)) return -1;
  char msg[200];
  if (ids_check(boards, n, h->B, h->id_role, msg, sizeof msg) != IDS_OK) return fail("td_step_boards: %s", msg);
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  StepArgs a = step_args(h, io);
  // td_retain_obs: a step into the retained buffer may skip what the buffer already holds of
  // the boards it steps; into any other buffer it leaves the retained buffer behind.
  const bool retained = h->ledger.is_retained(io->obs);
  const bool known = h->ledger.partial_step_skips(io->obs, boards, n);
  a.obs_skip = known ? 1 : 0;
  ObsLedger::Guard guard{&h->ledger};
  // on the stream: the refill and the ring guard, then the ids, then the kernel
  if (before_step_launch(h, a, s) || upload_ids(h, boards, nullptr, n, s)) return -1;
  const EvPair ev = next_timing_pair(h);  // whatever `every` is (as the copy's)
  HIP_OK(launch_step_sel(a, h->d_pairs, n, s, ev.e0, ev.e1));
  step_launched(h);
  if (!retained) h->ledger.touch();
  else
    for (int i = 0; !known && i < n; ++i) h->ledger.mark(boards[i]);  // written whole just now
  guard.ok = true;
  return 0;
}

// td_step_boards for a list, its length and its verdict in device memory: the host checks what it
// can see (the io, cap, the handle's settings), the check kernel the contents, on the stream in
// front of the list kernel; nothing is brought to the host and nothing is waited for.
int td_step_boards_dev(td_handle* h, const td_step_io* io, const int32_t* boards_dev, int cap, const int32_t* count_dev,
                       td_list_status* status_dev, void* stream) {
  const char* fn = "td_step_boards_dev";
  if (negative_cap_refused(fn, io, cap)) return -1;
  if (check_partial_step(fn, h, io)) return -1;
  if (const int go = check_list_args(fn, cap, h->B, boards_dev, "boards_dev"); go <= 0) return go;
  hipStream_t s = (hipStream_t)stream;
  StepArgs a = step_args(h, io);
  // td_retain_obs: which boards the list names is not known here, so the kernel skips clean
  // windows only if every board's row is known, and no board is marked afterwards
  a.obs_skip = h->ledger.list_step_skips(io->obs) ? 1 : 0;
  ObsLedger::Guard guard{&h->ledger};
  // on the stream: the refill and the ring guard, then the check, then the kernel
  if (before_step_launch(h, a, s) || enqueue_list_check(h, nullptr, boards_dev, cap, count_dev, status_dev, s)) return -1;
  const EvPair ev = next_timing_pair(h);  // the consumer's, whatever `every` is (as td_step_boards')
  HIP_OK(launch_step_list(a, boards_dev, cap, count_dev, &h->d_list->verdict, s, ev.e0, ev.e1));
  step_launched(h);
  h->ledger.list_call_into(io->obs);
  guard.ok = true;
  return 0;
}

// td_copy_boards for lists, their length and their verdict in device memory (see above).
int td_copy_boards_dev(td_handle* h, const int32_t* src_dev, const int32_t* dst_dev, int cap, const int32_t* count_dev,
                       float* obs, td_list_status* status_dev, void* stream) {
  const char* fn = "td_copy_boards_dev";
  if (cap < 0) return check_list_args(fn, cap, 0, false, "");  // (needs no handle)
  if (!h) return fail("%s: NULL handle", fn);
  if (const int go = check_list_args(fn, cap, h->B, src_dev && dst_dev, "src_dev or dst_dev"); go <= 0) return go;
  hipStream_t s = (hipStream_t)stream;
  ObsLedger::Guard guard{&h->ledger};
  if (enqueue_list_check(h, src_dev, dst_dev, cap, count_dev, status_dev, s)) return -1;
  StepArgs a = base_args(h);
  a.obs = obs;
  const EvPair ev = next_timing_pair(h);
  HIP_OK(launch_copy_list(a, src_dev, dst_dev, cap, count_dev, &h->d_list->verdict, s, ev.e0, ev.e1));
  // the destinations' states change: into the retained buffer the known boards stay known (their
  // rows were rewritten whole), any other buffer (or none) leaves it behind
  h->ledger.list_call_into(obs);
  guard.ok = true;
  return 0;
}

int td_list_errors(td_handle* h, td_list_status* first, int clear) {
  if (!h) return fail("td_list_errors: NULL handle");
  ListState ls;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(&ls, h->d_list, sizeof ls, hipMemcpyDeviceToHost));
  if (first) *first = ls.refused ? ls.first : td_list_status{0, 0, 0, 0};
  if (clear && ls.refused) {  // (key, arrived and verdict belong to the kernels)
    HIP_OK(hipMemset(&h->d_list->refused, 0, sizeof ls.refused));
    HIP_OK(hipMemset(&h->d_list->first, 0, sizeof ls.first));
  }
  return (int)std::min<uint32_t>(ls.refused, 0x7fffffffu);
}

// A kernel's name for its accessor: kept in the accessor's slot of the handle.
static const char* kept_name(td_handle* h, int slot, const std::string& name) {
  h->names[slot] = name;
  return h->names[slot].c_str();
}

const char* td_step_boards_dev_kernel_name(td_handle* h) {
  return h ? kept_name(h, NAME_LIST, kernel_display_name(list_row(base_args(h)))) : "";
}

const char* td_step_boards_kernel_name(td_handle* h) {
  return h ? kept_name(h, NAME_SEL, kernel_display_name(sel_row(base_args(h)))) : "";
}

void td_mask_io_init(td_mask_io* io) { io_init(io); }

namespace {

// What td_action_mask and its list forms check of their io, in this order, and the kernel
// arguments they make of it.  fn: the caller's name, for the message.
int check_mask_io(const char* fn, const td_handle* h, const td_mask_io* io, MaskArgs* out) {
  if (!io) return fail("%s: NULL io", fn);
  // the two header words first, as td_step
  if (io->size != (uint32_t)sizeof(td_mask_io) || io->abi != (uint32_t)TD_ABI_VERSION)
    return fail("%s: td_mask_io has size %u / abi %u, this library expects size %u / abi %d "
                "(call td_mask_io_init)", fn, io->size, io->abi, (unsigned)sizeof(td_mask_io), TD_ABI_VERSION);
  if (!h) return fail("%s: NULL handle", fn);
  if (!io->def_mask && !io->def_code && !io->atk_mask) return fail("%s: no output wanted (all three are NULL)", fn);
  const bool def_out = io->def_mask || io->def_code;
  if (def_out && h->mode == TD_MODE_ATK) return fail("%s: TD-atk has no defender side (def_mask / def_code)", fn);
  if (io->atk_mask && h->mode == TD_MODE_DEF) return fail("%s: TD-def has no attacker side (atk_mask)", fn);
  const size_t row = (size_t)6 * h->NC + (h->multi ? 0 : 1);
  size_t pitch = row;
  if (def_out && io->def_pitch != 0) {
    if (h->multi) return fail("%s: def_pitch must be 0 with multi-action (rows are [6][L][L], contiguous)", fn);
    if (io->def_pitch < row || io->def_pitch > kMaskMaxPitch)
      return fail("%s: def_pitch %zu outside [%zu, %zu] (6 L^2 + 1 bytes per row at L = %d)", fn, io->def_pitch, row,
                  kMaskMaxPitch, h->L);
    pitch = io->def_pitch;
  }
  *out = {board_view(h), io->def_mask, io->def_code, io->atk_mask, pitch};
  return 0;
}

}  // namespace

int td_action_mask(td_handle* h, const td_mask_io* io, void* stream) {
  MaskArgs a;
  if (check_mask_io("td_action_mask", h, io, &a)) return -1;
  HIP_OK(launch_mask(a, (hipStream_t)stream));
  return 0;
}

// td_action_mask for the boards named: the rows of every other board keep their bytes
// (td_mask_list.hip).
int td_action_mask_boards(td_handle* h, const td_mask_io* io, const int32_t* boards, int n, void* stream) {
  return read_boards("td_action_mask_boards", check_mask_io, launch_mask_list, h, io, boards, n, stream);
}

int td_action_mask_boards_dev(td_handle* h, const td_mask_io* io, const int32_t* boards_dev, int cap,
                              const int32_t* count_dev, td_list_status* status_dev, void* stream) {
  return read_boards_dev("td_action_mask_boards_dev", check_mask_io, launch_mask_list, h, io, boards_dev, cap, count_dev,
                         status_dev, stream);
}

const char* td_action_mask_boards_kernel_name(td_handle* h) {
  if (!h) return "";
  char buf[64];
  std::snprintf(buf, sizeof buf, "td_mask_list_kernel<%d>", with_side(h->L, [](auto lt) { return (int)decltype(lt)::value; }));
  return kept_name(h, NAME_MASK_LIST, buf);
}

void td_sample_io_init(td_sample_io* io) { io_init(io); }

namespace {

// What td_sample_actions and its list forms check of their io (td_call_check.h
// sample_io_refused), and the kernel arguments they make of it.  fn: the caller's name.
int check_sample_io(const char* fn, const td_handle* h, const td_sample_io* io, SampleArgs* out) {
  SampleIoSeen v;
  v.io = io != nullptr;
  if (io) { v.size = io->size; v.abi = io->abi; }
  v.handle = h != nullptr;
  if (sample_io_header_ok(v, (unsigned)sizeof(td_sample_io), TD_ABI_VERSION) && h) {
    v.mode = h->mode;
    v.def_act = io->def_act; v.atk_act = io->atk_act; v.def_count = io->def_count; v.atk_count = io->atk_count;
  }
  char msg[240];
  if (sample_io_refused(fn, v, (unsigned)sizeof(td_sample_io), TD_ABI_VERSION, msg, sizeof msg)) return fail("%s", msg);
  *out = {board_view(h), io->def_act, io->atk_act, io->def_count, io->atk_count, sample_key(io->seed, io->ticket),
          io->def_idle, io->atk_idle};
  return 0;
}

}  // namespace

// One kernel on the caller's stream; nothing is waited for.  Like the masks the calls only read
// state: no launch for the refill cadence or the ring guard, no timing pair, the observation
// ledger left alone.
int td_sample_actions(td_handle* h, const td_sample_io* io, void* stream) {
  SampleArgs a;
  if (check_sample_io("td_sample_actions", h, io, &a)) return -1;
  HIP_OK(launch_sample(a, nullptr, h->B, nullptr, nullptr, (hipStream_t)stream));
  return 0;
}

// The boards named, every other row left as it is.
int td_sample_actions_boards(td_handle* h, const td_sample_io* io, const int32_t* boards, int n, void* stream) {
  return read_boards("td_sample_actions_boards", check_sample_io, launch_sample, h, io, boards, n, stream);
}

int td_sample_actions_boards_dev(td_handle* h, const td_sample_io* io, const int32_t* boards_dev, int cap,
                                 const int32_t* count_dev, td_list_status* status_dev, void* stream) {
  return read_boards_dev("td_sample_actions_boards_dev", check_sample_io, launch_sample, h, io, boards_dev, cap, count_dev,
                         status_dev, stream);
}

const char* td_sample_actions_kernel_name(td_handle* h) {
  if (!h) return "";
  char buf[64];
  std::snprintf(buf, sizeof buf, "td_sample_kernel<%d>", with_side(h->L, [](auto lt) { return (int)decltype(lt)::value; }));
  return kept_name(h, NAME_SAMPLE, buf);
}

void td_sample_w_io_init(td_sample_w_io* io) { io_init(io); }

namespace {

// What td_sample_weighted and its list forms check of their io (td_call_check.h
// sample_w_io_refused), and the kernel arguments they make of it.  fn: the caller's name.
int check_sample_w_io(const char* fn, const td_handle* h, const td_sample_w_io* io, SampleWArgs* out) {
  SampleWIoSeen v;
  v.io = io != nullptr;
  if (io) { v.size = io->size; v.abi = io->abi; }
  v.handle = h != nullptr;
  if (sample_w_io_header_ok(v, (unsigned)sizeof(td_sample_w_io), TD_ABI_VERSION) && h) {
    v.mode = h->mode; v.multi = h->multi;
    v.def_act = io->def_act; v.atk_act = io->atk_act; v.def_w = io->def_w; v.atk_w = io->atk_w;
    v.def_mass = io->def_mass; v.atk_mass = io->atk_mass;
    v.def_w_aligned = (reinterpret_cast<uintptr_t>(io->def_w) & 3u) == 0;
    v.atk_w_aligned = (reinterpret_cast<uintptr_t>(io->atk_w) & 3u) == 0;
    v.pitch = io->def_w_pitch;
    v.row = (size_t)6 * h->NC + 1;
  }
  char msg[240];
  if (sample_w_io_refused(fn, v, (unsigned)sizeof(td_sample_w_io), TD_ABI_VERSION, kSampleWMaxPitch, msg, sizeof msg))
    return fail("%s", msg);
  *out = {board_view(h), io->def_act, io->atk_act, io->def_w, io->atk_w, io->def_mass, io->atk_mass,
          io->def_w_pitch ? io->def_w_pitch : v.row, sample_key(io->seed, io->ticket)};
  return 0;
}

}  // namespace

// td_sample_actions' three forms with the weighted kernel: one kernel on the caller's stream,
// nothing waited for, state only read.
int td_sample_weighted(td_handle* h, const td_sample_w_io* io, void* stream) {
  SampleWArgs a;
  if (check_sample_w_io("td_sample_weighted", h, io, &a)) return -1;
  HIP_OK(launch_sample_weighted(a, nullptr, h->B, nullptr, nullptr, (hipStream_t)stream));
  return 0;
}

int td_sample_weighted_boards(td_handle* h, const td_sample_w_io* io, const int32_t* boards, int n, void* stream) {
  return read_boards("td_sample_weighted_boards", check_sample_w_io, launch_sample_weighted, h, io, boards, n, stream);
}

int td_sample_weighted_boards_dev(td_handle* h, const td_sample_w_io* io, const int32_t* boards_dev, int cap,
                                  const int32_t* count_dev, td_list_status* status_dev, void* stream) {
  return read_boards_dev("td_sample_weighted_boards_dev", check_sample_w_io, launch_sample_weighted, h, io, boards_dev, cap,
                         count_dev, status_dev, stream);
}

const char* td_sample_weighted_kernel_name(td_handle* h) {
  if (!h) return "";
  char buf[64];
  std::snprintf(buf, sizeof buf, "td_sample_weighted_kernel<%d>",
                with_side(h->L, [](auto lt) { return (int)decltype(lt)::value; }));
  return kept_name(h, NAME_SAMPLE_W, buf);
}

void td_playout_io_init(td_playout_io* io) { io_init(io); }

namespace {

// What a playout's launch needs: the handle (the launch counts for its cadences), the step
// arguments with the io's outputs, and the playout's own.  The list is filled in at the launch.
struct PlayoutCall {
  td_handle* h;
  StepArgs a;
  PlayoutArgs p;
};

// What td_playout and its list forms check of their io and of the handle's settings
// (td_call_check.h playout_io_refused), and the call they make of it.  fn: the caller's name.
int check_playout_io(const char* fn, td_handle* h, const td_playout_io* io, PlayoutCall* out) {
  PlayoutIoSeen v;
  v.io = io != nullptr;
  if (io) { v.size = io->size; v.abi = io->abi; }
  v.handle = h != nullptr;
  if (playout_io_header_ok(v, (unsigned)sizeof(td_playout_io), TD_ABI_VERSION)) {
    v.steps = io->steps;
    v.reward = io->reward; v.done = io->done; v.first_def = io->first_def; v.first_atk = io->first_atk;
    if (h) { v.mode = h->mode; v.multi = h->multi; v.opp_np = h->opp_np; }
  }
  char msg[240];
  if (playout_io_refused(fn, v, (unsigned)sizeof(td_playout_io), TD_ABI_VERSION, TD_MAX_PLAYOUT_STEPS, msg, sizeof msg))
    return fail("%s", msg);
  out->h = h;
  StepArgs& a = out->a;
  a = base_args(h);
  a.frame_skip = io->steps;  // the sub-steps of this launch; td_frame_skip() plays no part
  a.reward = io->reward; a.done = io->done; a.win = io->win; a.allow_next = io->allow_next; a.cooldowns = io->cooldowns;
  a.ep_return = io->ep_return; a.ep_len = io->ep_len;
  a.ep_stats = h->d_epstats;
  a.last_ep = h->d_lastep;
  out->p = PlayoutArgs{};
  out->p.key0 = sample_sm(io->seed);
  out->p.ticket = io->ticket;
  out->p.def_idle = io->def_idle; out->p.atk_idle = io->atk_idle;
  out->p.steps_run = io->steps_run; out->p.first_def = io->first_def; out->p.first_atk = io->first_atk;
  return 0;
}

// The partial step's launch bracket, in td_step_boards[_dev]'s order on the stream: the refill at
// its cadence and the ring guard (playout_before), then the ids or the list check (read_boards,
// read_boards_dev), then the kernel with one timing pair, one launch counted and the retained
// observation left behind (the boards' states change and no row is written).  From the first
// enqueue on, a step that fails leaves the retained observation behind too, as ObsLedger::Guard
// does for the partial step.
int playout_before(const PlayoutCall& c, hipStream_t s) {
  if (before_step_launch(c.h, c.a, s)) {
    c.h->ledger.touch();
    return -1;
  }
  return 0;
}

// ids == nullptr: every board.
hipError_t launch_playout_call(const PlayoutCall& c, const int32_t* ids, int cap, const int32_t* count,
                               const td_list_status* verdict, hipStream_t s) {
  td_handle* const h = c.h;
  PlayoutArgs p = c.p;
  p.ids = ids; p.cap = cap; p.count = count; p.verdict = verdict;
  h->ledger.touch();
  const EvPair ev = next_timing_pair(h);  // whatever `every` is (as the list calls')
  const hipError_t e = launch_playout(c.a, p, cap, s, ev.e0, ev.e1);
  if (e == hipSuccess) step_launched(h);
  return e;
}

}  // namespace

// One kernel on the step's stream; nothing is waited for.
int td_playout(td_handle* h, const td_playout_io* io, void* stream) {
  PlayoutCall c;
  if (check_playout_io("td_playout", h, io, &c)) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (playout_before(c, s)) return -1;
  HIP_OK(launch_playout_call(c, nullptr, h->B, nullptr, nullptr, s));
  return 0;
}

// The boards named, every other board and output row left as it is.
int td_playout_boards(td_handle* h, const td_playout_io* io, const int32_t* boards, int n, void* stream) {
  return read_boards("td_playout_boards", check_playout_io, launch_playout_call, h, io, boards, n, stream, playout_before);
}

int td_playout_boards_dev(td_handle* h, const td_playout_io* io, const int32_t* boards_dev, int cap,
                          const int32_t* count_dev, td_list_status* status_dev, void* stream) {
  return read_boards_dev("td_playout_boards_dev", check_playout_io, launch_playout_call, h, io, boards_dev, cap, count_dev,
                         status_dev, stream, playout_before);
}

const char* td_playout_kernel_name(td_handle* h) {
  if (!h) return "";
  StepArgs a = base_args(h);
  a.multi = 0;  // (a multi-action handle is refused: the discrete row's name)
  return kept_name(h, NAME_PLAYOUT, kernel_display_name(playout_row(a)));
}

void td_probe_io_init(td_probe_io* io) { io_init(io); }

namespace {

// What a probe's launch needs: the handle (for the timing pair only), the step arguments with the
// io's outputs, and the probe's own.  The list is filled in at the launch.
struct ProbeCall {
  td_handle* h;
  StepArgs a;
  ProbeArgs q;
};

// What td_probe and its list forms check of their io and of the handle's settings: the playout's
// refusals with the replicas behind the steps (td_call_check.h playout_io_refused), and the call
// they make of it.  fn: the caller's name.
int check_probe_io(const char* fn, td_handle* h, const td_probe_io* io, ProbeCall* out) {
  PlayoutIoSeen v;
  v.io = io != nullptr;
  if (io) { v.size = io->size; v.abi = io->abi; }
  v.handle = h != nullptr;
  if (playout_io_header_ok(v, (unsigned)sizeof(td_probe_io), TD_ABI_VERSION)) {
    v.steps = io->steps; v.reps = io->reps;
    v.reward = io->reward; v.done = io->done; v.first_def = io->first_def; v.first_atk = io->first_atk;
    if (h) { v.mode = h->mode; v.multi = h->multi; v.opp_np = h->opp_np; }
  }
  char msg[240];
  const ProbeIoLimit lim{TD_MAX_PROBE_REPS};
  if (playout_io_refused(fn, v, (unsigned)sizeof(td_probe_io), TD_ABI_VERSION, TD_MAX_PLAYOUT_STEPS, msg, sizeof msg, &lim))
    return fail("%s", msg);
  out->h = h;
  StepArgs& a = out->a;
  a = base_args(h);
  a.frame_skip = io->steps;  // the sub-steps of a replica; td_frame_skip() plays no part
  a.reward = io->reward; a.done = io->done; a.win = io->win;  // [B][reps]; no other step output, no episode record
  out->q = ProbeArgs{};
  PlayoutArgs& p = out->q.p;
  p.key0 = sample_sm(io->seed);
  p.ticket = io->ticket;
  p.def_idle = io->def_idle; p.atk_idle = io->atk_idle;
  p.steps_run = io->steps_run; p.first_def = io->first_def; p.first_atk = io->first_atk;
  out->q.reps = io->reps;
  return 0;
}

// The kernel with one timing pair and nothing else: state is only read, so no refill, no ring
// guard, no launch counted, the observation ledger left alone (as the masks and the sampler).
// ids == nullptr: every board.
hipError_t launch_probe_call(const ProbeCall& c, const int32_t* ids, int cap, const int32_t* count,
                             const td_list_status* verdict, hipStream_t s) {
  ProbeArgs q = c.q;
  q.p.ids = ids; q.p.cap = cap; q.p.count = count; q.p.verdict = verdict;
  const EvPair ev = next_timing_pair(c.h);  // whatever `every` is (as the list calls')
  return launch_probe(c.a, q, cap, s, ev.e0, ev.e1);
}

}  // namespace

// One kernel on the step's stream; nothing is waited for, nothing of the handle is written.
int td_probe(td_handle* h, const td_probe_io* io, void* stream) {
  ProbeCall c;
  if (check_probe_io("td_probe", h, io, &c)) return -1;
  HIP_OK(launch_probe_call(c, nullptr, h->B, nullptr, nullptr, (hipStream_t)stream));
  return 0;
}

// The boards named, every other output row left as it is.
int td_probe_boards(td_handle* h, const td_probe_io* io, const int32_t* boards, int n, void* stream) {
  return read_boards("td_probe_boards", check_probe_io, launch_probe_call, h, io, boards, n, stream);
}

int td_probe_boards_dev(td_handle* h, const td_probe_io* io, const int32_t* boards_dev, int cap, const int32_t* count_dev,
                        td_list_status* status_dev, void* stream) {
  return read_boards_dev("td_probe_boards_dev", check_probe_io, launch_probe_call, h, io, boards_dev, cap, count_dev,
                         status_dev, stream);
}

const char* td_probe_kernel_name(td_handle* h) {
  if (!h) return "";
  StepArgs a = base_args(h);
  a.multi = 0;  // (a multi-action handle is refused: the discrete row's name)
  return kept_name(h, NAME_PROBE, kernel_display_name(probe_row(a)));
}

// Both kernel-kind setters: the kind is checked against the map side (td_kernel_choice.h
// kernel_kind_ok), forced for both kinds of launch or for skipping launches only
// (KernelChoice::force_both, force_retained), and the kinds are resolved again.
static int set_kernel_kind(const char* fn, td_handle* h, int kind, void (KernelChoice::*force)(int)) {
  if (!h) return fail("NULL handle");
  char msg[200];
  if (!kernel_kind_ok(fn, kind, h->L, msg, sizeof msg)) return fail("%s", msg);
  HIP_OK(hipDeviceSynchronize());  // launches already queued keep the kernel they were enqueued with
  (h->kernel.*force)(kind);
  return apply_kernel(h);
}

int td_set_step_kernel(td_handle* h, int kind) {
  return set_kernel_kind("td_set_step_kernel", h, kind, &KernelChoice::force_both);
}

int td_set_retained_step_kernel(td_handle* h, int kind) {
  return set_kernel_kind("td_set_retained_step_kernel", h, kind, &KernelChoice::force_retained);
}

int td_step_kernel(td_handle* h) { return h ? h->kernel.small + 1 : fail("NULL handle"); }

int td_retained_step_kernel(td_handle* h) { return h ? h->kernel.small_retained + 1 : fail("NULL handle"); }

// The observation's element.  A kernel kind the caller forced stays, TD_KERNEL_AUTO is
// resolved again for the new format (apply_kernel), for both kinds of launch; the write-through
// policy and the kernel's name follow the new byte size.
int td_set_obs_format(td_handle* h, int fmt) {
  if (!h) return fail("NULL handle");
  if (fmt != TD_OBS_F32 && fmt != TD_OBS_F16) return fail("td_set_obs_format: unknown format %d (TD_OBS_F32 = 0, TD_OBS_F16 = 1)", fmt);
  HIP_OK(hipDeviceSynchronize());  // launches already queued keep the format they were enqueued with
  h->obs_fmt = fmt;
  h->ledger.touch();  // (the same format again too: the caller may have changed the buffer's element)
  return apply_kernel(h);
}

int td_obs_format(td_handle* h) { return h ? h->obs_fmt : fail("NULL handle"); }

// Board steps per td_step.  No board state changes and the retained observation stays
// known: only the kernel td_step launches, and its name, follow k.
int td_set_frame_skip(td_handle* h, int k) {
  if (!h) return fail("NULL handle");
  if (k < 1 || k > TD_MAX_FRAME_SKIP)
    return fail("td_set_frame_skip: k = %d outside [1, %d] (TD_MAX_FRAME_SKIP)", k, TD_MAX_FRAME_SKIP);
  if (k > 1 && h->multi) return fail("td_set_frame_skip: k = %d > 1 is not supported on a multi-action handle", k);
  if (k > 1 && h->opp_np) return fail("td_set_frame_skip: k = %d > 1 is not supported with random_agent=False", k);
  HIP_OK(hipDeviceSynchronize());  // launches already queued keep the kernel they were enqueued with
  h->frame_skip = k;
  return apply_kernel(h);
}

int td_frame_skip(td_handle* h) { return h ? h->frame_skip : fail("NULL handle"); }

size_t td_obs_bytes(td_handle* h) {
  return h ? (size_t)h->B * NCH * h->NC * (h->obs_fmt == TD_OBS_F16 ? 2u : 4u) : 0;
}

int td_retain_obs(td_handle* h, const void* obs) {
  if (!h) return fail("NULL handle");
  HIP_OK(hipDeviceSynchronize());  // launches already queued keep what they were enqueued with
  h->ledger.retained = obs;
  h->ledger.touch();  // nothing is known of the buffer yet: the next step into it writes every byte
  return 0;
}

const void* td_retained_obs(td_handle* h) { return h ? h->ledger.retained : nullptr; }

// The kernel of the most recent td_step; before it, and after a kernel, format or frame-skip
// change, the kernel of a launch that writes every window (apply_kernel).
const char* td_step_kernel_name(td_handle* h) {
  if (!h) return "";
  const StepArgs a = base_args(h);
  return kept_name(h, NAME_STEP, kernel_display_name(h->frame_skip > 1 ? skip_row(a) : step_row(a, h->kernel.name_kind)));
}

int td_set_refill_interval(td_handle* h, int steps) {
  if (!h || steps < 0) return fail("td_set_refill_interval: bad arguments");
  h->refill_every = steps;
  return 0;
}

int td_kernel_timing(td_handle* h, int max_launches, int every) {
  if (!h || max_launches < 0 || every < 1) return fail("td_kernel_timing: bad arguments");
  HIP_OK(hipDeviceSynchronize());
  // Timing events without the system-scope release at the timed kernel's end: the cache
  // write-back it implies lengthens the very kernel being timed (4,096 boards: sampled
  // kernels 21.9 us = the 21.9-us step with it, 20.6 us in a 21.3-us step without;
  // profiles/r04/s2).
  const unsigned flags = hipEventDisableSystemFence;
  while ((int)h->tev.size() < 2 * max_launches) {
    hipEvent_t e = nullptr;
    HIP_OK(hipEventCreateWithFlags(&e, flags));
    h->tev.push_back(e);
  }
  h->tev_cap = max_launches;
  h->tev_n = 0;
  h->tev_every = every;
  h->tev_from = h->steps;
  return 0;
}

int td_kernel_times(td_handle* h, float* us, int cap) {
  if (!h || (cap > 0 && !us)) return fail("td_kernel_times: bad arguments");
  const int n = h->tev_n;
  for (int i = 0; i < n && i < cap; ++i) {
    HIP_OK(hipEventSynchronize(h->tev[2 * (size_t)i + 1]));
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, h->tev[2 * (size_t)i], h->tev[2 * (size_t)i + 1]));
    us[i] = ms * 1000.0f;
  }
  return n;
}

int td_episode_stats(td_handle* h, double* dev_out, int clear, void* stream) {
  if (!h || !dev_out) return fail("td_episode_stats: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  HIP_OK(hipMemcpyAsync(dev_out, h->d_epstats, 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (clear) HIP_OK(hipMemsetAsync(h->d_epstats, 0, 2 * sizeof(double), s));
  return 0;
}

int td_opponent(td_handle* h, int side, int level, const uint8_t* host_mask, void* stream) {
  if (!h) return fail("NULL handle");
  if (side == 0 && (level < 0 || level > 1)) return fail("td_opponent: random_enemy_lv%d does not exist", level);
  if (side == 1 && (level < 0 || level > 2)) return fail("td_opponent: random_tower_lv%d does not exist", level);
  if (side != 0 && side != 1) return fail("td_opponent: side must be 0 (enemy) or 1 (tower)");
  hipStream_t s = (hipStream_t)stream;
  HIP_OK(hipDeviceSynchronize());
  if (upload_mask(h, host_mask)) return -1;
  StepArgs a = base_args(h);
  a.reset_mask = h->d_mask;
  h->ledger.touch();  // enemies, towers and costs change; no observation is written
  HIP_OK(launch_opponent(a, side, level, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

int td_episode_records(td_handle* h, td_episode_record* dev_out, void* stream) {
  if (!h || !dev_out) return fail("td_episode_records: NULL argument");
  HIP_OK(hipMemcpyAsync(dev_out, h->d_lastep, (size_t)h->B * sizeof(td_episode_record), hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
  return 0;
}

int td_layout_words(int map_size) { return layout_words(map_size); }

int td_layout_from_roads(int map_size, int num_roads, const int32_t* cells, const int32_t* offsets, uint32_t* rec) {
  int st = layout_from_roads(map_size, num_roads, cells, offsets, rec);
  return st == ROAD_OK ? 0 : fail("td_layout_from_roads: invalid roads (status %d)", st);
}

int td_layout_generate(uint32_t* np_state625, int map_size, int max_attempts, uint32_t* rec) {
  if (map_size < 4 || map_size > MAX_L) return fail("map_size out of range");
  std::vector<uint8_t> scratch(road_scratch_bytes(map_size));
  return episode_layout(np_state625, map_size, scratch.data(), max_attempts > 0 ? max_attempts : kRoadAttempts, rec);
}

size_t td_state_bytes(td_handle* h, int count) {
  if (!h || count < 0) return 0;
  return state_rec_bytes(h->NC, (size_t)count);
}

// The record (td_state_rec.h) to or from the boards [b0, b0 + count): one copy per record array.
static int state_copy(td_handle* h, int b0, int count, void* host, bool to_host) {
  if (!h || b0 < 0 || count < 0 || b0 + count > h->B) return fail("state copy: bad board range");
  HIP_OK(hipDeviceSynchronize());
  uint8_t* p = (uint8_t*)host;
  std::vector<uint8_t> retagged;
  if (!to_host) {  // the caller's record stays as it is: a copy takes the current config epoch
    retagged.assign(p, p + state_rec_bytes(h->NC, (size_t)count));
    p = retagged.data();
    state_rec_retag(p, h->NC, (size_t)count, h->epoch);
  }
  uint32_t* opp = (uint32_t*)(p + state_rec_offset(SR_OPP_MT, h->NC, (size_t)count));
  std::vector<uint32_t> hot((size_t)count * HOT_WORDS);
  if (!to_host) {  // the hot record follows the imported words (no pre-drawn outputs)
    state_rec_pos_to_hot(opp, hot.data(), HOT_WORDS, (size_t)count);
    HIP_OK(hipMemcpy(h->d_hot + (size_t)b0 * HOT_WORDS, hot.data(), hot.size() * 4, hipMemcpyHostToDevice));
  }
  void* const dev[SR_ARRAYS] = {h->d_hdr,   h->d_en_lp,  h->d_en_mg, h->d_en_inf,
                                h->d_tw_cd, h->d_tw_inf, h->d_cells, h->d_opp};  // in record order
  for (int k = 0; k < SR_ARRAYS; ++k) {
    const size_t elem = state_rec_elem(k, h->NC), bytes = (size_t)count * elem;
    uint8_t* d = (uint8_t*)dev[k] + (size_t)b0 * elem;
    uint8_t* r = p + state_rec_offset(k, h->NC, (size_t)count);
    HIP_OK(hipMemcpy(to_host ? (void*)r : (void*)d, to_host ? (void*)d : (void*)r, bytes,
                     to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice));
  }
  if (to_host) {  // position and lazy boundary live in the hot record
    HIP_OK(hipMemcpy(hot.data(), h->d_hot + (size_t)b0 * HOT_WORDS, hot.size() * 4, hipMemcpyDeviceToHost));
    state_rec_pos_from_hot(opp, hot.data(), HOT_WORDS, (size_t)count);
  }
  return 0;
}

int td_export_state(td_handle* h, int b0, int count, void* host_dst) { return state_copy(h, b0, count, host_dst, true); }

// The headers are checked before anything is copied (td_state_rec.h state_rec_check).
int td_import_state(td_handle* h, int b0, int count, const void* host_src) {
  if (!h || !host_src || b0 < 0 || count < 0 || b0 + count > h->B) return fail("td_import_state: bad arguments");
  char msg[200];
  if (state_rec_check(static_cast<const TdHdr*>(host_src), count, b0, msg, sizeof msg))
    return fail("td_import_state: %s", msg);
  h->ledger.touch();
  return state_copy(h, b0, count, const_cast<void*>(host_src), false);
}

int td_get_flags(td_handle* h, int32_t* host_flags) {
  if (!h || !host_flags) return fail("td_get_flags: NULL argument");
  std::vector<TdHdr> hdr((size_t)h->B);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(hdr.data(), h->d_hdr, hdr.size() * sizeof(TdHdr), hipMemcpyDeviceToHost));
  for (int b = 0; b < h->B; ++b) host_flags[b] = hdr[(size_t)b].flags;
  return 0;
}



// Diagnostic: hold (1) or give back (0) board b's refill claim, as a refill wave drawing
// its layouts would (tests: a claim held past the ring guard's 1-s wait).
int td_debug_set_claim(td_handle* h, int b, int held) {
  if (!h || b < 0 || b >= h->B) return fail("td_debug_set_claim: bad board");
  HIP_OK(hipDeviceSynchronize());
  const uint32_t v = held ? 1u : 0u;
  HIP_OK(hipMemcpy(h->d_lay_claim + b, &v, 4, hipMemcpyHostToDevice));
  return 0;
}

int td_guard_timeouts(td_handle* h, int clear) {
  if (!h) return fail("NULL handle");
  uint32_t n = 0;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(&n, h->d_guard_to, 4, hipMemcpyDeviceToHost));
  if (clear) HIP_OK(hipMemset(h->d_guard_to, 0, 4));
  return (int)std::min<uint32_t>(n, 0x7fffffffu);
}

int td_set_store_policy(td_handle* h, int xcd_map, int edge_wt) {
  if (!h || (xcd_map != 0 && xcd_map != 1) || (edge_wt != 1 && edge_wt != 2))
    return fail("td_set_store_policy: xcd_map must be 0 / 1 and edge_wt 1 / 2");
  HIP_OK(hipDeviceSynchronize());
  h->xcd_map = xcd_map;
  h->edge_wt = edge_wt;
  return 0;
}

int td_board_map(int n_boards, int kind, int xcd_map, int32_t* out) {
  if (n_boards < 1 || !out || kind < 0 || kind > 1) return fail("td_board_map: bad arguments");
  for (int i = 0; i < n_boards; ++i)
    out[i] = xcd_map ? xcd_board(i, n_boards) : i;
  return 0;
}

void td_py_seed(uint32_t* mt, uint32_t seed) { py_seed(mt, seed); }
void td_np_seed(uint32_t* mt, uint32_t seed) { np_seed(mt, seed); }
uint32_t td_mt_next(uint32_t* mt) { return MtRef{mt}.next(); }
int64_t td_py_randint(uint32_t* mt, int64_t a, int64_t b) { return MtRef{mt}.py_randint(a, b); }
int64_t td_np_randint(uint32_t* mt, int64_t lo, int64_t hi) { return MtRef{mt}.np_randint(lo, hi); }

}  // extern "C"
