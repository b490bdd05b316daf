/* tdstep.h -- C-ABI of the MI355X-native batched gym-TD step (libtdstep.so).
 *
 * The reference (LiuTed/gym-TD) is pure Python: its only boundary is the gym.Env
 * surface.  Each entry point below replaces one piece of that surface for a batch
 * of B independent boards that live in HBM; the Python mirror
 * (gym-td_amd/gym_TD) binds them with ctypes:
 *
 *   td_create / td_destroy     TDGymBasic.__init__            gym_TD/envs/TDGymBasic.py:18-28
 *                              TDDefense/TDAttack/TDMulti.__init__ (TDDefense.py:19-26,
 *                              TDAttack.py:18-22, TDMulti.py:16-31)
 *   td_set_config              paramConfig                    gym_TD/envs/TDParam.py:98-100
 *   td_seed                    TDGymBasic.seed                TDGymBasic.py:30-32 (+ the opponent's
 *                              `random` stream, TDGymBasic.py:84-86,98-100)
 *   td_reset                   TDGymBasic.reset               TDGymBasic.py:37-55
 *   td_step                    TDDefense.step / TDAttack.step / TDMulti.step
 *                              (TDDefense.py:34-87, TDAttack.py:27-56, TDMulti.py:46-138)
 *                              -> TDBoard.step/done/get_states (TDBoard.py:295-385, 85-144)
 *   td_layout_generate         TDRoadGen.create_road_v2       TDRoadGen.py:4-199 (+ map planes
 *                              TDBoard.py:31-59)
 *   td_layout_from_roads       TDBoard.__init__ map planes    TDBoard.py:31-59
 *   td_export_state / import   the board's Python attributes (enemies, towers, costs, map[6])
 *
 * Conventions
 *   - every array argument of td_step / td_reset is a caller-owned DEVICE pointer
 *     (e.g. a torch tensor's data_ptr()), work is enqueued on `stream` (a
 *     hipStream_t, NULL = default stream) and the call returns immediately;
 *   - one handle per stream/thread; handles are not thread-safe;
 *   - int return codes: 0 = OK, < 0 = error (td_last_error() has the message);
 *     nothing throws across the ABI;
 *   - per-board error bits (capacity overflow, invalid action, missing layout)
 *     are kept on the device, read them with td_get_flags().
 */
#ifndef TDSTEP_H_
#define TDSTEP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 3: td_step_io starts with its own size and ABI words, which td_step checks before
 * it reads anything else (an ABI-2 struct -- 14 pointers, no header -- is refused).
 * ABI 2: td_step_io.cooldowns.  ABI 1: the first release. */
#define TD_ABI_VERSION 3

enum td_mode { TD_MODE_DEF = 0, TD_MODE_ATK = 1, TD_MODE_2P = 2 };

/* TD_FLAG_BAD_ACTION, the rule (the reference asserts on such input; this is the device's own,
 * pinned by tests/test_gpu_bad_action.py).  Actions are int64 and all 64 bits count.
 *   discrete defender   an action outside 0 .. 6 L^2 becomes 6 L^2, the empty action:
 *                       real_def = 6 L^2, fail_def = 0
 *   attacker            each entry outside 0 .. 4 becomes 4 ("none") -- that entry, not its
 *                       cluster; real_atk shows 4 there
 *   multi-action flags  each flag outside 0 .. 2 counts as 0; its real-action entry is 0
 * The board's flag word gains TD_FLAG_BAD_ACTION in that step, whether or not the side is
 * cooling down, and the step then runs exactly as with the sanitised action.  No other board
 * is touched.  Like every flag it survives an auto-reset and is cleared by an explicit reset
 * (td_reset / td_reset_layouts) of that board.
 *
 * TD_FLAG_BAD_MOVE: a layout whose road dead-ends away from the end cell (against the layout
 * rule at td_layout_from_roads) sends an enemy towards a position outside the board.  The
 * step tests the position before it forms a cell index: the move is not made -- the enemy
 * keeps its cell, with the margin already reduced by 1, and moves no further in that step --
 * and the board's flag word gains TD_FLAG_BAD_MOVE in that step.  (The reference indexes its
 * map with the position: an IndexError, or a wrap to the other edge.)  No other board is
 * touched; td_reset / td_reset_layouts of that board clear the flag. */
enum td_board_flag {
  TD_FLAG_EN_OVERFLOW = 1, /* more than 128 live enemies: summon refused */
  TD_FLAG_TW_OVERFLOW = 2, /* more than 32 towers: build refused */
  TD_FLAG_BAD_ACTION = 4,  /* an action value outside the action space: sanitised, see above */
  TD_FLAG_NO_LAYOUT = 8,   /* auto-reset found no staged layout */
  TD_FLAG_BAD_MOVE = 16,   /* an enemy's move would leave the board (a dead-end road): not made, see above */
  TD_FLAG_CLAIM_TIMEOUT = 32 /* a wait for the board's refill claim gave up after 1 s: the ring
                                guard left its ring short, or its episode end found no layout
                                (then TD_FLAG_NO_LAYOUT too); see td_guard_timeouts */
};

/* Game parameters: gym_TD/envs/TDParam.py:1-64 (Config) and :105-111 (HyperParameters).
 * Numbers are doubles so Python ints and floats both round-trip exactly.
 *   What the device represents, field by field (td_create returns NULL and td_set_config < 0,
 * with the message in td_last_error and nothing changed -- no new config epoch, a retained
 * observation stays retained -- for anything else; the checks are gym-td_amd/csrc/td_cfg_check.h):
 *   - the nine tables and every rate, cost, reward and ratio: any finite double, used as it is
 *     (enemy_LP > 0).  A NaN or an infinity in ANY double field is refused.
 *   - frozen_time (0 .. 255), base_LP (1 .. 2^31 - 1), tower_distance (0 .. 15),
 *     attacker_action_interval and defender_action_interval (0 .. 2^31 - 1): the device keeps
 *     them as integers, so the value must be one.  A fraction is refused, not truncated: the
 *     reference computes with the float (frozen_time = 2.5 slows an enemy for three marches,
 *     TDBoard.py:322-324, a truncated 2 for two), which no integer reproduces in the state
 *     export and the observation alike.
 *   - tower_distance may not grow while a board holds a tower (td_set_config only; < 0, nothing
 *     changed).  The reference subtracts a destructed tower's diamond at the current
 *     tower_distance (TDBoard.py:281-287): wider than the one it added, it takes map[6] below zero,
 *     and to zero under another tower, where a second tower may then be built on the same cell.
 *     A cell holds an unsigned count and one tower, so the change that leads there is refused;
 *     reset the boards (or destruct the towers) first.  A smaller tower_distance is always taken.
 *   - max_tower_lv 0 or 1.  The observation has 45 planes either way: with max_tower_lv = 0 the
 *     reference's has 44 (one tower-level plane, TDBoard.py:129,154); here plane 16 is then all
 *     zero and every other channel keeps its index. */
typedef struct td_config {
  double enemy_LP[4][2], enemy_speed[4][2], enemy_defense[4][2], enemy_cost[4][2];
  double tower_attack[4][2], tower_range[4][2], tower_splash_range[4][2];
  double tower_cost[4][2], tower_attack_interval[4][2];
  double tower_destruct_return, frozen_time, frozen_ratio;
  double attacker_init_cost, defender_init_cost, base_LP, max_cost;
  double reward_kill, penalty_leak, reward_time;
  double attacker_cost_init_rate, attacker_cost_final_rate, defender_cost_rate;
  double tower_distance, enemy_upgrade_at;
  double attacker_action_interval, defender_action_interval;
  int32_t max_enemy_lv, max_tower_lv, enemy_types, tower_types;
  int32_t max_episode_steps, max_cluster_length, max_num_of_roads, reserved;
} td_config;

/* Device outputs of one step.  Only obs/reward/done (and the action inputs the
 * mode needs) are required; every other pointer may be NULL.
 *   def_act   int64 [B] (discrete) or [B][6][L][L] (multi-action)   TD-def, TD-2p
 *   atk_act   int64 [B][3][8]                                       TD-atk, TD-2p
 *   obs       float [B][45][L][L]   reward double [B]   done uint8 [B]
 *   real_def  int64 [B] or [B][6][L][L]   real_atk int64 [B][3][8]   info['RealAction']
 *   fail_def  int32 [B]   fail_atk int32 [B][3] (-1 = no entry)       info['FailCode']
 *   win       int8 [B] (-1 = None)                                     info['Win']
 *   allow_next uint8 [B] (bit0 attacker_cd<=1, bit1 defender_cd<=1)   info['AllowNextMove']
 *             (bits 2-7 are always 0)
 *   ep_return double [B], ep_len int32 [B]: running episode return / length after this
 *             step (the finished episode's totals when done[b]).
 *   cooldowns uint8 [B]: the env's attacker_cd (bits 0-3) and defender_cd (bits 4-7) after the
 *             step (TDDefense.py:38-39,75, TDAttack.py:31-32,44), each saturated at 15
 *             (ABI 2; ABI 1 packed them into allow_next bits 2-7).
 *   size, abi: sizeof(td_step_io) and TD_ABI_VERSION as the caller was built (ABI 3;
 *             td_step_io_init sets both).  td_step reads these two words first and refuses,
 *             with no launch, a struct whose size or ABI differs from its own: a caller
 *             built against another layout of this struct is caught, not stepped. */
typedef struct td_step_io {
  uint32_t size;
  uint32_t abi;
  const int64_t* def_act;
  const int64_t* atk_act;
  float* obs;
  double* reward;
  uint8_t* done;
  int64_t* real_def;
  int64_t* real_atk;
  int32_t* fail_def;
  int32_t* fail_atk;
  int8_t* win;
  uint8_t* allow_next;
  double* ep_return;
  int32_t* ep_len;
  uint8_t* cooldowns;
} td_step_io;

typedef struct td_handle td_handle;

/* The observation's element, per engine.  TD_OBS_F32 (the default): float [B][45][L][L].
 * TD_OBS_F16: IEEE binary16, _Float16 [B][45][L][L], dense, same index order -- each value
 * is the float32 value of the default format rounded to nearest-even (one conversion in
 * front of the store; the board work and the channel arithmetic are the same, and every
 * other output is unchanged).  After td_set_obs_format(h, TD_OBS_F16) every entry point
 * that writes an observation -- td_step, its auto-reset, the reset kernel behind a step
 * with random_agent = 0, td_reset, td_reset_layouts -- takes its `obs` pointer (declared
 * float* here and in td_step_io, whose layout does not change) to be that _Float16 array
 * of td_obs_bytes(h) bytes.
 *   Alignment: 2 B is enough.  An 8-B-aligned buffer takes the line-aligned store path at
 * L = 10 / 20 / 30 (8-B stores, one quad of cells per lane) and the small kernels; an
 * 8-B-aligned buffer at any other L with L^2 % 4 == 0 the quad path of the generic kernel;
 * anything else the per-element path (same bytes, slower).  (float32: 16 B, as td_step.)
 *   td_set_obs_format synchronises the device first, as the mode setters do, and may be
 * called at any time between steps; it changes no board state.  A kernel kind forced
 * with td_set_step_kernel stays; TD_KERNEL_AUTO is resolved again for the new format (with
 * half the bytes to store, 10x10 boards above half a round step fastest on SMALL: the
 * boards in flight bound the step, not the store stream).  The write-through store policy
 * follows the new byte size, and td_step_kernel_name
 * returns "td_step_kernel_f16<...>", "td_step_kernel_small_f16<...>" or
 * "td_step_kernel_small2_f16<...>" (the float32 kernels keep their names).  An unknown fmt
 * returns < 0 and changes nothing.  td_obs_bytes: B * 45 * L * L * element size. */
enum td_obs_format { TD_OBS_F32 = 0, TD_OBS_F16 = 1 };
int td_set_obs_format(td_handle* h, int fmt);
int td_obs_format(td_handle* h);
size_t td_obs_bytes(td_handle* h);

/* Retained observation (off by default: td_retain_obs(h, NULL)).  The caller promises
 * that from now on the td_obs_bytes(h) bytes at `obs` are changed only by this handle's own
 * calls that are given that same pointer: td_step, its auto-reset, the reset kernel behind
 * a step with random_agent = 0, td_reset and td_reset_layouts.  The library may then leave
 * unwritten any byte it knows to equal what its last write left there: a td_step into the
 * retained buffer writes, per board, only the 1-KB windows that hold a channel of a class
 * that may have changed -- the costs, progress and channels 41-44 always; the enemy planes
 * if the board has an enemy before or after the step; channel 5 after a leak; channels 21-24
 * when cost_def crosses a tower cost; the tower planes when the tower list changed; the
 * layout planes only with a new episode.  The buffer then holds exactly what a full write
 * would have left.  (Read it, copy from it; writing into it breaks the promise.)
 *   What may be skipped is tracked per handle: a step skips only if its io->obs is the
 * retained pointer and every board's observation is known to be in it.  That knowledge is
 * gained by a td_step into the retained buffer (the first one writes every byte), or board
 * by board by td_reset / td_reset_layouts into it (once every board was reset there), and lost
 * by every call that changes what some board's observation would be without writing it
 * there: td_retain_obs itself, td_set_config, td_set_obs_format, td_import_state,
 * td_opponent, a td_reset / td_reset_layouts with another or a NULL obs, a td_step with
 * another obs, and any of these calls that fails.  (td_reset / td_reset_layouts into the
 * retained buffer write the boards they reset whole and keep it; the setters that change
 * no observation byte -- auto-reset, random_agent, seeds and stream states, the refill
 * interval, the step kernel and the store policy -- keep it too.)  td_free_device(p) drops
 * the retention of every live handle whose retained address lies in block p, so an address
 * a later allocation reuses is never taken for the old buffer; memory from any other
 * allocator must be un-retained by the caller before it is freed.  The per-element paths
 * (an obs that is not 16-B / 8-B aligned, L other than 10 / 20 / 30) always write every byte.
 *   td_retain_obs synchronises the device first.  td_retained_obs: the pointer, or NULL. */
int td_retain_obs(td_handle* h, const void* obs);
const void* td_retained_obs(td_handle* h);

/* Frame skip (an extension; off by default: k = 1, and nothing changes).  With k > 1 one
 * td_step is a macro step: every board runs up to k board steps ("sub-steps") in one launch
 * and ONE observation is written -- the observation's cost per board step becomes 1 / k.
 *   Sub-step 0 takes the caller's actions exactly as a step does (FLAG_BAD_ACTION included);
 * sub-steps 1 .. k-1 take the empty action for every side the caller controls (defender:
 * 6 L^2, attacker: all 4s), as the reference's trainer steps when no move is allowed.  The
 * built-in opponents act in every sub-step on the board's own stream and the cool-downs
 * decrement every sub-step, as in k separate steps.  A board stops after the sub-step that
 * finishes its episode; with auto-reset its new episode starts there (at most one staged
 * layout per board per launch).
 *   Outputs: reward = r0, then the f64 sum left to right over the executed sub-steps
 * (TD-atk: each already negated); done, win, allow_next, cooldowns, ep_return, ep_len = what
 * the last executed sub-step would have written (ep_len and td_episode_records keep
 * counting board steps); real_def / fail_def / real_atk / fail_atk = sub-step 0's, the only
 * one that carried an action; board flags are OR-ed; obs = the state after the last executed
 * sub-step (after an auto-reset: the new episode's first observation), written once in the
 * handle's format and store policy.  With td_retain_obs "before" is the board as loaded at
 * the start of the macro step.  On a board where no sub-step finishes an episode, state,
 * both RNG streams and every output equal those of k steps (action, empty, ..., empty).
 *   td_set_frame_skip may be called between any two steps (it synchronises the device
 * first) and changes no board state.  Refused (< 0, td_last_error, nothing changed):
 * k outside 1 .. TD_MAX_FRAME_SKIP; k > 1 on a multi-action handle; k > 1 with
 * random_agent = 0 -- and td_set_random_agent(h, 0) while k > 1.  While k > 1 td_step
 * launches "td_skip_kernel<L, mode>" / "td_skip_kernel_f16<L, mode>" (td_step_kernel_name)
 * whatever kind td_set_step_kernel chose; that choice is kept for k = 1.  The refill cadence
 * and the ring guard count launches, and td_kernel_timing times the launch. */
#define TD_MAX_FRAME_SKIP 16
int td_set_frame_skip(td_handle* h, int k);
int td_frame_skip(td_handle* h);

int td_abi_version(void);
/* sizeof(td_step_io) as this library was built (120 on LP64 at ABI 3). */
int td_step_io_size(void);
/* Device memory for a caller's output buffers (the observation above all), zeroed;
 * contiguous != 0: physically contiguous where the driver can give it
 * (hipDeviceMallocContiguous), else a plain allocation.  A contiguous observation stepped
 * 4-5 % faster than a default allocation at 10x10 / 65,536 and 20x20 / 30x30 boards in
 * one probe (profiles/r04/s24); TDEngine's choice is TD_CONTIG_OBS (gym_TD/engine.py).
 * The reference allocates its observation per call (np.zeros in TDBoard.get_states,
 * gym_TD/envs/TDBoard.py:85-112); no counterpart.  td_free_device releases it (after the
 * work that writes it is done). */
int td_alloc_device(size_t bytes, int device, int contiguous, void** out);
int td_free_device(void* p);
/* How td_alloc_device placed block p: 1 physically contiguous, 0 a plain allocation (a
 * contiguous request the driver refused falls back to one), -1 not a live td_alloc_device
 * block.  (A placement a caller records -- e.g. to key a measurement by it -- is this one,
 * not the request.) */
int td_alloc_is_contiguous(const void* p);
/* Zero *io and set its size / abi words (a C caller's initialiser; writes td_step_io_size()
 * bytes, so io must be this header's td_step_io). */
void td_step_io_init(td_step_io* io);
const char* td_last_error(void);
void td_config_default(td_config* cfg);

/* Device memory per board: ~8.2 KB + 18*L^2 B of state (records, both RNG streams, the
 * layout draw's scratch) plus a ring of 16 staged layouts of (8 + L^2 rounded up to 32)
 * words each -- ~18 KB at L = 10 (1.2 GB at 65,536 boards), ~84 KB at L = 30 (5.5 GB at
 * 65,536).  A failed allocation names the footprint in td_last_error(). */
/* mode: td_mode; multi_action: HyperParameters.allow_multiple_actions;
 * difficulty: built-in opponent level (TD-def: 0/1, TD-atk: 0/1/2, TD-2p: ignored);
 * map_size: 10/20/30 have specialised kernels, any 4 <= L <= 32 works. */
td_handle* td_create(const td_config* cfg, int map_size, int n_boards, int mode, int multi_action,
                     int difficulty, int device);
void td_destroy(td_handle* h);
/* paramConfig on a live engine (TDParam.py:98-100): values the reference reads live from
 * `config` change from the next step; enemies and towers keep the stats they were created
 * or upgraded with (TDElements.py:4-69, 134-170) and each board the max_cost / base_LP of
 * its last reset (TDBoard.py:66-72) -- the device keeps one constant block per config
 * epoch (up to 256 still referenced by live entities).  td_config_epoch: the current one. */
int td_set_config(td_handle* h, const td_config* cfg);
int td_config_epoch(td_handle* h);
int td_set_autoreset(td_handle* h, int on);
/* TDGymBasic(random_agent=...) (TDGymBasic.py:18-26): with random_agent = 0 the built-in
 * opponents draw from each board's numpy layout stream (np_random, :87-89,101-103,
 * 118-120,139-160,176-177,188-190,213-256) instead of its CPython stream; the destruct
 * branch's tower index stays on CPython random (:191, :287).  Play and reset() then
 * share the stream in order: with auto-reset on, a finished board's next layout is drawn
 * right after the step that ended its episode (a second kernel on the step's stream), as
 * gym's AsyncVectorEnv calls reset() there; nothing is staged ahead.  Switching to 0 is
 * refused while a board holds layouts an auto-reset refill drew ahead of play (set it
 * before the first reset, or re-seed with td_seed).  Both mode setters synchronise the
 * device first. */
int td_set_random_agent(td_handle* h, int random_agent);

/* Board b's layout stream = numpy.random.RandomState(np_seeds[b]) and its built-in
 * opponent stream = random.Random(py_seeds[b]).  Host arrays of n_boards entries. */
int td_seed(td_handle* h, const uint32_t* np_seeds, const uint32_t* py_seeds);
/* CPython `random.getstate()` import/export for one board: 624 words + position. */
int td_set_py_state(td_handle* h, int board, const uint32_t* mt625);
int td_get_py_state(td_handle* h, int board, uint32_t* mt625);
int td_set_np_state(td_handle* h, int board, const uint32_t* mt625);
int td_get_np_state(td_handle* h, int board, uint32_t* mt625);

/* Start a new episode on every board with host_mask[b] != 0 (NULL = all): draws
 * the layout from the board's numpy stream (on the device; with auto-reset on, a
 * layout staged ahead of time by the refill kernel is used), resets the board and
 * writes its initial observation into obs (device, may be NULL).  Synchronous.
 * Returns the number of boards whose road generation failed (the reference raises
 * or hangs there, TDRoadGen.py:177-189); those boards keep their previous state. */
int td_reset(td_handle* h, const uint8_t* host_mask, float* obs, void* stream);

/* Boards whose road generation failed in the last td_reset (ids into boards[0..cap)); returns the count. */
int td_last_reset_failures(td_handle* h, int32_t* boards, int cap);

/* Reset from explicit layout records (td_layout_words(L) uint32 each, host memory), as
 * td_layout_from_roads / td_layout_generate make them.  A record without the magic word, with
 * num_roads (word 1) outside 1 .. 3 or with max dist (word 3) above 63 -- the step kernels'
 * distance table has 64 entries -- is refused (< 0, td_last_error) before anything is copied
 * or launched: no board, flag or retained observation changes.  The cell words of a record
 * are taken as they are. */
int td_reset_layouts(td_handle* h, const uint32_t* recs, const int32_t* boards, int n, float* obs, void* stream);

/* Copy board states on the device: after the call's work has run on `stream`, board dst[i] of
 * this handle is board src[i], for every i in [0, n) -- the fork a search needs (expanding a
 * node, rollouts from a common root, restarting a population from its best board).  The
 * reference has no counterpart short of copy.deepcopy(env); the host form of the same is
 * td_export_state + td_import_state, which waits for the device, retags the entities to the
 * current config epoch, drops the pre-drawn opponent outputs and voids the retained observation.
 * src / dst: host arrays of n board ids; they are the caller's again when the call returns.
 * Copied, per pair: the whole 96-B header (flags, episodes, ep_return, cool-downs and the
 *   captured max_cost / max_base_LP: the clone carries its source's history); the live enemy
 *   slots [0, n_en) and tower slots [0, n_tw) (counts from the source's header, clamped to 128 /
 *   32; slots at or past the count are unspecified, as after any step), config-epoch tags as
 *   they are -- both boards read this handle's config blocks, and td_set_config counts the
 *   clone's entities when it recycles a block; the L^2 cell words; the opponent's 626 stream
 *   words and its hot record, pre-drawn outputs included.
 * Not copied: with random_agent = 1 the destination keeps its own layout stream, staged
 *   layouts and pending draw -- a fork is its source until the episode ends, then starts the
 *   next episode of its OWN layout sequence.  With random_agent = 0 the numpy stream is the
 *   opponent's too and nothing is staged ahead, so it is copied as well: the fork stays its
 *   source through auto-resets.  The last-finished-episode records (td_episode_records) and the
 *   episode statistics are never touched, nor is any td_step_io output of an earlier step.
 * obs (device, may be NULL): the whole observation of every destination is written into row
 *   dst[i], in the handle's format and with td_step's element and alignment rules -- what a full
 *   write of that state under the current config leaves: bytewise the source's row after the
 *   step that produced the state, unless td_set_config came between (which voids a retained
 *   observation anyway).  The row of a destination whose source holds no episode (never successfully reset)
 *   is left unwritten, as td_reset leaves the row of a board whose draw failed.  With
 *   obs == td_retained_obs(h) the buffer stays retained and the rows written count as known;
 *   any other obs, NULL included, leaves the retained buffer behind (the next step into it
 *   writes every byte), as does a call that fails after its checks.
 * Asynchronous on `stream`, which must be the step's stream (as for td_action_mask); the
 *   device is not waited for.  (The ids are staged through four pinned slots of the handle in
 *   turn; only a call issued while the upload four calls back is still pending waits, for that
 *   upload.)  n == 0 returns 0 and launches nothing.
 * Refused (< 0, td_last_error; checked on the host before anything is enqueued, so no board,
 *   flag, observation byte or retention state changes): a NULL handle; NULL arrays with n > 0;
 *   n < 0 or n > the handle's boards; an id outside [0, boards); a board named twice in dst; a
 *   board named in both src and dst (the result would depend on pair order).  A board repeated
 *   in src is the point of the call: one root, many children. */
int td_copy_boards(td_handle* h, const int32_t* src, const int32_t* dst, int n, float* obs, void* stream);

/* One env step for all boards (asynchronous on `stream`).  Buffers need only their
 * element type's alignment; a 16-B-aligned obs (and, multi-action, 16-B-aligned flag
 * and real-action arrays) takes the line-aligned 16-B store path, any other the
 * per-element one (same bytes, slower). */
int td_step(td_handle* h, const td_step_io* io, void* stream);

/* One env step for the boards boards[0 .. n) only -- exactly the step td_step would have given
 * each of them -- while every other board keeps every byte of its state, both RNG streams, its
 * staged layouts and its flags: the other half of a search iteration beside td_copy_boards (fork
 * the leaves, step the leaves, read their rows and masks), as a reference user steps exactly the
 * env objects they choose (copy.deepcopy(env), then child.step(a)).
 * io: td_step's struct, with the same required pointers and the same size / abi check made
 *   first.  Every array keeps its full-batch shape and is indexed by board id: actions are read
 *   from the rows of the named boards only, and outputs (obs, reward, done, real / fail, win,
 *   allow_next, cooldowns, ep_return, ep_len) are written to those rows only -- no byte of an
 *   unnamed row changes, the observation lines it shares with a named neighbour included.
 *   td_episode_stats / td_episode_records count and record the named boards only.
 * boards: a host array of n board ids, the caller's again when the call returns (staged through
 *   td_copy_boards' four pinned slots and uploaded on `stream` in front of the kernel).  Order
 *   is free and the results do not depend on it.  n == 0 returns 0, launches nothing and counts
 *   as no launch.
 * The kernel: one wave per named board in td_step's TD_KERNEL_LARGE shape, whatever kind
 *   td_step launches (td_step_boards_kernel_name); an obs buffer unaligned for its
 *   format takes the per-element path, as in td_step.  A named board that was never reset
 *   behaves as in td_step: zero row, done = 1, TD_FLAG_NO_LAYOUT.
 * The call counts as a launch for the refill cadence and the ring guard (a board consumes at
 *   most one staged layout per launch, whether the launch steps every board or some), and with
 *   td_kernel_timing pairs left its kernel takes the next pair, whatever `every` is.
 * Retained observation: with io->obs == td_retained_obs(h) the kernel skips clean windows only
 *   if every named board's row is known to hold its last observation; afterwards the named
 *   boards' rows are known and the buffer stays retained.  A step into any other buffer leaves
 *   the retained buffer behind (the next step into it writes every byte), as td_step does.
 * Asynchronous on `stream`, which must be the step's stream.
 * Refused (< 0, td_last_error; checked on the host before anything is enqueued, so no board,
 *   flag, observation byte or retention state changes): a NULL handle or io, or a bad size / abi
 *   word; missing required pointers; NULL boards with n > 0; n < 0 or n > the handle's boards;
 *   an id outside [0, boards); an id named twice (two waves on one board would race);
 *   td_frame_skip() > 1; random_agent = 0 with auto-reset on (the reset kernel behind a step
 *   goes by done[] of every board, and an unnamed board's is stale). */
int td_step_boards(td_handle* h, const td_step_io* io, const int32_t* boards, int n, void* stream);

/* Device-resident board lists: td_step_boards and td_copy_boards for a search whose ids are on
 * the device already (the argmax of a score, "every board that is not done", the best k of a
 * population), with no copy to the host, no wait for the stream and no O(n) host check.  The
 * list and its length are read from device memory; the validation runs in a kernel on the
 * step's stream (td_list_check_kernel) in front of the kernel that consumes the list; a list
 * the device refuses makes every wave of that kernel exit before it reads or writes anything of
 * any board, and the refusal is reported after the fact (status_dev, td_list_errors).
 * For a list the device accepts the result is byte for byte what td_step_boards /
 * td_copy_boards give for the same ids: board state, both RNG streams, flags, every output row,
 * the episode statistics and records.  io, obs, the outputs and the kernel shape (one wave per
 * list entry in TD_KERNEL_LARGE's shape; td_step_boards_dev_kernel_name) are those of the
 * host-list forms, and so is the accounting: a call counts as a launch for the refill cadence
 * and the ring guard, and its consumer kernel takes the next td_kernel_timing pair.
 * boards_dev / src_dev / dst_dev: cap int32 ids in device memory.
 * count_dev: device memory, may be NULL = cap entries are used.  Otherwise the first *count_dev
 *   entries are used, which must lie in [0, cap]; entries at or past the count are never read
 *   as ids, whatever they hold -- a caller compacts "the boards that are not done" into a
 *   buffer of fixed size without learning the count on the host.  The grid is cap either way.
 * Lifetime of the id memory: what these pointers name must be final, in stream order, before
 *   the call (written by earlier work on `stream`, or complete on the host's side), and must
 *   stay unchanged until the call's kernels have run; work enqueued on the same stream after
 *   the call may reuse it.
 * status_dev (device, may be NULL): the call's verdict, written on every call that launches,
 *   code = TD_LIST_OK on success.  call: the 0-based serial of the device-list calls of this
 *   handle that launched (a call refused on the host, or with cap == 0, has no serial).  code:
 *   the lowest-numbered defect class present in the list.  entry / board: one list entry that
 *   shows that defect and the id it holds (for TD_LIST_TWICE and TD_LIST_OVERLAP any one of the
 *   entries that name the board); for TD_LIST_BAD_COUNT entry is -1 and board the count read.
 * Refused on the host (< 0, td_last_error, nothing enqueued, nothing changed): a NULL io or a
 *   bad size / abi word, then a NULL handle, in td_step's order and with the call's own name;
 *   missing required pointers; a NULL id array with cap > 0; cap < 0 (needs no handle: checked
 *   with the io words) or cap > the handle's boards; for the step td_frame_skip() > 1 and
 *   random_agent = 0 with auto-reset on, for td_step_boards' reasons.  cap == 0 returns 0 and
 *   launches nothing.
 * Refused on the device -- everything about the contents: a count outside [0, cap]
 *   (TD_LIST_BAD_COUNT); an id outside [0, boards) (TD_LIST_RANGE); a board named twice in
 *   boards or in dst (TD_LIST_TWICE); a board named in both src and dst (TD_LIST_OVERLAP).  A
 *   board repeated in src is fine, as in td_copy_boards.  Then nothing changes: no board, flag,
 *   stream, output row, observation byte, retained window, episode statistic or record.  (The
 *   side refill and the ring guard in front of a step launch may still have run; they never
 *   change a result.)  The call itself returned 0: read status_dev in stream order, or ask
 *   td_list_errors.
 * Retained observation: the host does not know which boards a call names.  A step into
 *   td_retained_obs(h) skips clean windows only if EVERY board's row is known; where the set
 *   was not complete the named rows are written whole, but the set of known boards stays as it
 *   was.  A copy into the retained buffer leaves the set unchanged too (a known destination's
 *   row was just rewritten whole, an unknown one stays unknown).  A step or copy into any other
 *   buffer, and a copy with obs == NULL, leaves the retained buffer behind (the next step into
 *   it writes every byte), as the host-list forms do -- even if the device then refuses the
 *   list; that costs one full write.  A device refusal never makes the handle claim more than
 *   it did.
 * Asynchronous on `stream`, which must be the step's stream. */
enum td_list_code { TD_LIST_OK = 0, TD_LIST_BAD_COUNT = 1, TD_LIST_RANGE = 2, TD_LIST_TWICE = 3, TD_LIST_OVERLAP = 4 };
typedef struct td_list_status { int32_t code, call, entry, board; } td_list_status; /* 16 B */
int td_step_boards_dev(td_handle* h, const td_step_io* io, const int32_t* boards_dev, int cap,
                       const int32_t* count_dev, td_list_status* status_dev, void* stream);
/* td_copy_boards for a device-resident list: board dst_dev[i] becomes board src_dev[i] for the
 * entries used, obs as in td_copy_boards.  Everything else -- cap and count_dev, the lifetime
 * of the id memory, status_dev, the refusal split between host (a NULL handle, NULL arrays
 * with cap > 0, cap < 0 or > the handle's boards) and device (TD_LIST_BAD_COUNT, TD_LIST_RANGE,
 * TD_LIST_TWICE in dst, TD_LIST_OVERLAP of src and dst), the retained-observation rules (the
 * set of known boards is unchanged by a copy into td_retained_obs(h); any other obs, NULL
 * included, leaves the retained buffer behind) and the td_kernel_timing pair -- is as the
 * comment above td_step_boards_dev says.  Asynchronous on `stream`, the step's stream. */
int td_copy_boards_dev(td_handle* h, const int32_t* src_dev, const int32_t* dst_dev, int cap,
                       const int32_t* count_dev, float* obs, td_list_status* status_dev, void* stream);
/* How many device-list calls (td_step_boards_dev, td_copy_boards_dev, td_action_mask_boards_dev) the device refused since
 * the last clear, and in *first (may be NULL) the record of the first of them; with no refusal
 * *first is all zero (code = TD_LIST_OK).  clear != 0 zeroes the count and the record.  Waits
 * for the device's work first -- synchronous, the pattern of td_guard_timeouts: a search loop
 * asks once in a while, not per call. */
int td_list_errors(td_handle* h, td_list_status* first, int clear);

/* Legal-action masks: for every board and every action, whether the NEXT td_step would
 * execute that action if it were the only thing asked of that side -- decided on the device
 * from the board's present state with the step's own comparisons, so a policy can sample
 * legal moves only (the reference reports legality after the fact, info['FailCode'] /
 * ['RealAction']; its trainer's one-bit form is AllowNextMove, train/main.py:130-132).
 * A td_set_config between the mask and the step voids the mask.
 *   def_mask  uint8, discrete [B][def_pitch]: entry a in [0, 6 L^2], a = op * L^2 + cell
 *             (TDDefense.py:65-67).  The no-op a = 6 L^2 is always 1; any other a is 1 iff the
 *             defender's cool-down is <= 1 (the gate of TDDefense.py:39,64 after the decrement)
 *             and the operation would return fail code 0.  Bytes [6 L^2 + 1, def_pitch) are
 *             written as 0.  Multi-action: [B][6][L][L], each entry = that flag alone would
 *             succeed (flags set together interact: out of scope).
 *   def_code  uint8, same shape: the fail code the operation would return, the cool-down
 *             aside, tested in the step's order -- build: 1 cost (TDBoard.py:228), 2 position
 *             (:232), 6 the device's 32-tower capacity; level-up: 4 no tower (:269-271),
 *             3 level (:252), 1 cost (:256, current config epoch); destruct: 4 no tower.
 *             The no-op and the padding read 0.  def_mask == (def_code == 0 && cool-down <= 1)
 *             except the no-op.
 *   atk_mask  uint8 [B][3][5]: entry (road, t).  t = 4 (none) is always 1; t < 4 is 1 iff
 *             road < num_roads, the attacker's cool-down is <= 1, fewer than 128 enemies live
 *             and cost_atk >= enemy_cost[t][lv], lv as the header's steps give it
 *             (steps / max_episode_steps >= enemy_upgrade_at, TDBoard.py:201).
 *   def_pitch discrete: bytes between rows, 0 = 6 L^2 + 1, else >= 6 L^2 + 1 (and <= 65,536);
 *             multi-action: must be 0.  Rows whose start and pitch are multiples of 16 are
 *             stored in 16-B pieces throughout (same bytes at any alignment).
 * A board that was never reset (its road generation failed) has only the always-legal entries.
 * NULL = not wanted; an output for a side the mode lacks, all three NULL, a bad pitch or a
 * size / abi mismatch (checked first, as td_step) return < 0 and launch nothing.
 * Asynchronous on `stream`, which must be the step's stream: the kernel reads the state the
 * last td_step (and, with random_agent = 0 and auto-reset, the reset kernel behind it, on
 * that stream too) left, and writes nothing but these outputs. */
typedef struct td_mask_io {
  uint32_t size;
  uint32_t abi;
  uint8_t* def_mask;
  uint8_t* def_code;
  uint8_t* atk_mask;
  size_t def_pitch;
} td_mask_io;
/* Zero *io and set its size / abi words. */
void td_mask_io_init(td_mask_io* io);
int td_action_mask(td_handle* h, const td_mask_io* io, void* stream);

/* td_action_mask for the boards a list names: the third call of a search iteration, beside
 * td_copy_boards (fork the leaves) and td_step_boards (step the leaves), in both of their
 * flavours.  io is td_action_mask's, unchanged: the outputs keep their full-batch shape and are
 * indexed by board id -- def_mask, def_code, atk_mask, def_pitch, the multi-action [B][6][L][L]
 * form, any alignment.  Row b of every wanted output is written for every named board b, byte
 * for byte what td_action_mask writes there; no byte of an unnamed row changes, the 16-B pieces
 * and 128-B lines it shares with a named neighbour included (a pitch that is no multiple of 16,
 * the 15-B attacker rows).
 * The calls write nothing but these outputs: no board, RNG stream or flag changes, the
 * retained-observation ledger is not touched, they are no launch for the refill cadence or the
 * ring guard, and they take no td_kernel_timing pair (as td_action_mask takes none).  One wave
 * per list entry, several entries per workgroup (td_action_mask_boards_kernel_name).
 * Asynchronous on `stream`, which must be the step's stream.
 * td_action_mask_boards -- a host list, under td_step_boards' rules: order free, the array is
 *   the caller's again on return, n == 0 returns 0 and launches nothing.  Refused (< 0,
 *   td_last_error with the call's name; on the host, before anything is enqueued, so no output
 *   byte changes), in this order: a NULL io, a bad size / abi word, a NULL handle, no output
 *   wanted, an output for a side the mode lacks, a bad pitch (all as td_action_mask); n < 0 or
 *   n > the handle's boards; NULL boards with n > 0; an id outside [0, boards); an id named
 *   twice.  Unlike the step, td_frame_skip() > 1 and random_agent = 0 with auto-reset are no
 *   reason to refuse: the kernel only reads state.
 * td_action_mask_boards_dev -- a device list, under td_step_boards_dev's contract word for word
 *   where it applies: cap and count_dev, the lifetime of the id memory, status_dev, and the
 *   split of the refusals.  On the host: td_action_mask's refusals with this call's name, cap
 *   < 0 (with the io words, before the handle), cap > the handle's boards, NULL boards_dev with
 *   cap > 0; cap == 0 returns 0 and launches nothing.  On the device (td_list_check_kernel in
 *   front, the call takes the next serial of the handle's device-list calls):
 *   TD_LIST_BAD_COUNT, TD_LIST_RANGE, TD_LIST_TWICE -- then no output byte is written, the call
 *   returned 0, and td_list_errors counts the refusal. */
int td_action_mask_boards(td_handle* h, const td_mask_io* io, const int32_t* boards, int n, void* stream);
int td_action_mask_boards_dev(td_handle* h, const td_mask_io* io, const int32_t* boards_dev, int cap,
                              const int32_t* count_dev, td_list_status* status_dev, void* stream);
/* The kernel both calls launch, as rocprofv3 shows it: "td_mask_list_kernel<10>" (L, or 0 for a
 * generic side).  The string is the handle's, valid until the next call. */
const char* td_action_mask_boards_kernel_name(td_handle* h);

/* One uniformly drawn legal action per side and board, on the device: what a random-legal
 * baseline, the default policy of a rollout or the exploring branch of an epsilon-greedy trainer
 * would otherwise make of td_action_mask's rows on their own.  The candidates are the entries
 * td_action_mask would mark 1, the always-legal ones aside:
 *   defender, discrete      a in [0, 6 L^2) with def_mask[a] == 1, in ascending a; n_def of them
 *                           (0 while the cool-down is closed and on a board never reset).  The
 *                           action is 6 L^2 (the no-op) if n_def == 0 or the idle draw fires,
 *                           else the k-th candidate.
 *   defender, multi-action  the legal flags of [6][L][L] in flat order; the output row is written
 *                           whole: zeros, and a single 1 at the chosen flag where one is chosen.
 *   attacker                the pairs (road, t < 4) with atk_mask[road][t] == 1 in ascending
 *                           road * 4 + t; the output [3][8] is all 4, and [road][0] = t where a
 *                           pair is chosen.
 * One candidate per side and call, so the step executes what was sampled: RealAction is the
 * sampled action and FailCode 0 (several flags at once interact: out of scope, as for the mask).
 * The randomness is stateless -- splitmix64 over (seed, ticket, board id, draw):
 *   sm(z): z += 0x9E3779B97F4A7C15; z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *          z *= 0x94D049BB133111EB; z ^= z >> 31
 *   word(seed, ticket, b, j) = sm(sm(sm(seed) + ticket) + 4 b + j),  u = word >> 32
 *   j = 0: the defender idles iff u < def_idle;  j = 1: its pick k = (u * n_def) >> 32
 *   j = 2: the attacker idles iff u < atk_idle;  j = 3: its pick k = (u * n_atk) >> 32
 * (bias of the pick <= n / 2^32, n <= 6,144; no rejection loop).  A call writes nothing but its
 * outputs -- no board, RNG stream, flag, ledger or refill cadence changes --, is reproducible,
 * and two copies of one board at different ids draw differently: vary `ticket` per call.
 *   def_act    int64, td_step_io.def_act's format ([B] or [B][6][L][L]); NULL = not wanted
 *   atk_act    int64 [B][3][8]; NULL = not wanted
 *   def_count  int32 [B] n_def, atk_count int32 [B] n_atk; may be NULL (the log-probability of a
 *              pick is -log n)
 *   def_idle, atk_idle  probability of choosing nothing although something is legal, in units
 *              of 2^-32; 0 = only when nothing is legal
 * Refused (< 0, nothing launched), in this order: a NULL io, a bad size / abi word, a NULL
 * handle, no action output wanted (def_act and atk_act both NULL), an output or count for a side
 * the mode lacks.  Asynchronous on `stream`, which must be the step's stream; nothing is waited
 * for.  The calls take no td_kernel_timing pair and are no launch for the refill cadence.
 * td_sample_actions_boards / _boards_dev -- the list forms, under td_action_mask_boards[_dev]'s
 *   contract word for word: the arrays keep their full-batch shape and are indexed by board id
 *   (the layout td_step_boards reads), only the named rows are written, and the row of a named
 *   board is the row td_sample_actions gives that board under the same seed and ticket (the key
 *   is the board id, not the list position).  Host list: n < 0 or n > the handle's boards, NULL
 *   boards with n > 0, an id out of range or named twice are refused on the host; n == 0
 *   returns 0.  Device list: cap < 0 (with the io words, before the handle), cap > the handle's
 *   boards and NULL boards_dev on the host; TD_LIST_BAD_COUNT, TD_LIST_RANGE, TD_LIST_TWICE on
 *   the device (td_list_check_kernel in front, the next serial of the handle's device-list
 *   calls): then no output byte is written, the call returned 0 and td_list_errors counts it.
 *   td_frame_skip() > 1 and random_agent = 0 are no reason to refuse. */
typedef struct td_sample_io {
  uint32_t size, abi;          /* checked first, as td_step_io / td_mask_io */
  int64_t* def_act;
  int64_t* atk_act;
  int32_t* def_count;
  int32_t* atk_count;
  uint64_t seed, ticket;
  uint32_t def_idle, atk_idle;
} td_sample_io;
/* Zero *io and set its size / abi words. */
void td_sample_io_init(td_sample_io* io);
int td_sample_actions(td_handle* h, const td_sample_io* io, void* stream);
int td_sample_actions_boards(td_handle* h, const td_sample_io* io, const int32_t* boards, int n, void* stream);
int td_sample_actions_boards_dev(td_handle* h, const td_sample_io* io, const int32_t* boards_dev, int cap,
                                 const int32_t* count_dev, td_list_status* status_dev, void* stream);
/* The kernel the three calls launch, as rocprofv3 shows it: "td_sample_kernel<10>" (L, or 0 for
 * a generic side).  The string is the handle's, valid until the next call. */
const char* td_sample_actions_kernel_name(td_handle* h);

/* One legal action per side and board drawn in proportion to caller-supplied weights, on the
 * device: the link between a policy's output tensor (a network's action distribution, PUCT
 * priors, a heuristic prior) and td_step, where td_sample_actions serves the uniform policy.
 * The rule is exact -- integers only, so the result does not depend on how the sum is taken:
 *   weights  float32, meant in [0, 1]: probabilities, or exp(logit - row max)
 *   q(w)     0 unless w > 0 (NaN, -0, negatives and 0 give 0), else
 *            (uint32) trunc(min(w, 1.0f) * 2^31): +inf and everything above 1 give 2^31,
 *            subnormals and everything below 2^-31 give 0
 *   defender, discrete handles only: entries a in [0, 6 L^2]; m(a) = q(def_w[b][a]) where a is
 *            6 L^2 (the no-op, always legal) or a candidate of td_sample_actions
 *            (td_action_mask's def_mask[a] == 1), else 0.  S = sum of m(a), a uint64 < 2^44.
 *            S == 0: the no-op.  Else r = (word(seed, ticket, b, 1) * S) >> 64 -- the whole
 *            64-bit word of td_sample_actions' draw j = 1, a 64 x 64 -> 128-bit product -- and
 *            the action is the smallest a whose inclusive prefix sum of m exceeds r.
 *   attacker entries e in [0, 12]: e < 12 is the pair (road, t) = (e >> 2, e & 3), legal iff
 *            atk_mask[road][t] == 1; e = 12 is "summon nothing", always legal.  Weights
 *            atk_w[b][13], draw j = 3, the same rule.  The output [3][8] is all 4 but the chosen
 *            road's first slot, as td_sample_actions writes it.
 *   mass     on request, per side: uint64 [B][2] = (m(chosen), S), or (0, 0) when S == 0.  The
 *            pick's probability is m / S, up to a multiply-shift bias of at most S / 2^64 < 2^-20
 *            (log-probability: log m - log S).
 * Idling is part of the distribution (the no-op's weight, entry 12): there is no def_idle /
 * atk_idle, and draws 0 and 2 are unused.  The key is td_sample_actions': the board id, not the
 * list position -- a weighted and a uniform call at the same (seed, ticket) share words: vary
 * `ticket` per call.  One candidate per side, so the step executes what was sampled: RealAction
 * is the sampled action and FailCode 0.  While the defender's cool-down is closed, and on a
 * board never reset, only the always-legal entry can carry mass: the result is the no-op and the
 * weight row is not read (but its last float, for the mass).  A call writes nothing but its
 * outputs -- no board, RNG stream, flag, ledger or refill cadence changes.
 *   def_act    int64 [B]; NULL = not wanted        atk_act   int64 [B][3][8]; NULL = not wanted
 *   def_w      float32 [B][def_w_pitch], entry a of board b at def_w[b * def_w_pitch + a]
 *   atk_w      float32 [B][13]
 *   def_mass, atk_mass   uint64 [B][2]; may be NULL
 *   def_w_pitch  floats between rows; 0 = 6 L^2 + 1, else >= 6 L^2 + 1 and <= 65,536
 * The weight pointers need 4-byte alignment only; the result is the same at any alignment of the
 * rows, and nothing behind a row's 6 L^2 + 1 (13) floats is read.
 * Refused (< 0, nothing launched), in this order: a NULL io, a bad size / abi word, a NULL
 * handle, no action output wanted, any pointer of a side the mode lacks, an action output
 * without its weights or a mass without its action, a weight pointer that is no multiple of 4, a
 * bad pitch, the defender side on a multi-action handle (the attacker side of such a handle is
 * served).  Asynchronous on `stream`, which must be the step's stream; nothing is waited for.
 * The calls take no td_kernel_timing pair and are no launch for the refill cadence.
 * td_sample_weighted_boards / _boards_dev -- the list forms, under
 *   td_sample_actions_boards[_dev]'s contract word for word: the arrays, weights included, keep
 *   their full-batch shape and are indexed by board id, only the named rows are written, and the
 *   row of a named board is the row td_sample_weighted gives that board under the same seed and
 *   ticket.  Host list: n < 0 or n > the handle's boards, NULL boards with n > 0, an id out of
 *   range or named twice are refused on the host; n == 0 returns 0.  Device list: cap < 0 (with
 *   the io words, before the handle), cap > the handle's boards and NULL boards_dev on the host;
 *   TD_LIST_BAD_COUNT, TD_LIST_RANGE, TD_LIST_TWICE on the device (td_list_check_kernel in
 *   front, the next serial of the handle's device-list calls): then no output byte is written,
 *   the call returned 0 and td_list_errors counts it.  td_frame_skip() > 1 and random_agent = 0
 *   are no reason to refuse. */
typedef struct td_sample_w_io {
  uint32_t size, abi;          /* checked first, as td_step_io / td_sample_io */
  int64_t* def_act;
  int64_t* atk_act;
  const float* def_w;
  const float* atk_w;
  uint64_t* def_mass;
  uint64_t* atk_mass;
  size_t def_w_pitch;
  uint64_t seed, ticket;
} td_sample_w_io;
/* Zero *io and set its size / abi words. */
void td_sample_w_io_init(td_sample_w_io* io);
int td_sample_weighted(td_handle* h, const td_sample_w_io* io, void* stream);
int td_sample_weighted_boards(td_handle* h, const td_sample_w_io* io, const int32_t* boards, int n, void* stream);
int td_sample_weighted_boards_dev(td_handle* h, const td_sample_w_io* io, const int32_t* boards_dev, int cap,
                                  const int32_t* count_dev, td_list_status* status_dev, void* stream);
/* The kernel the three calls launch, as rocprofv3 shows it: "td_sample_weighted_kernel<10>" (L,
 * or 0 for a generic side).  The string is the handle's, valid until the next call. */
const char* td_sample_weighted_kernel_name(td_handle* h);

/* Random playouts: up to `steps` board steps ("sub-steps") of every board in ONE launch, under
 * the uniform random legal policy, with no observation written -- what a Monte-Carlo search
 * spends its time in.  Everything is defined by calls the library already has.  Sub-step j
 * (j = 0, 1, ...) of a board is exactly this pair:
 *   td_sample_actions with (seed, ticket + j mod 2^64, def_idle, atk_idle) for every side the
 *     caller controls, on the board's state before the sub-step (the key is the board id);
 *   one td_step_boards step of that board with those actions.
 * TD-def: the defender is sampled and the built-in attacker acts on the board's own stream;
 * TD-atk: the attacker is sampled and the built-in defender acts; TD-2p: both sides are sampled
 * from the same pre-state, as one td_sample_actions call gives them.
 *   A board stops after the sub-step that ends its episode; with auto-reset its new episode
 *     starts there (frame skip's rule: at most one staged layout per launch; a ring found dry
 *     is waited for as in td_step, and TD_FLAG_NO_LAYOUT where no layout comes).
 *   A board never reset gets reward 0, done 1, steps_run 0 and TD_FLAG_NO_LAYOUT, and nothing
 *     else of it changes (win -1, allow_next 0, cooldowns 0, ep_return 0, ep_len 0; first_def
 *     the no-op, first_atk all 4).
 *   What is sampled is legal: a playout never sets TD_FLAG_BAD_ACTION and every sub-step's
 *     FailCode is 0.
 * After the call the board's exported state, the opponent's stream (td_get_py_state; for a board
 * whose episode did not end also the raw words and the lazy-twist boundary), the flags (OR-ed),
 * td_episode_stats and td_episode_records equal those of the loop of td_sample_actions_boards +
 * td_step_boards over the boards not yet done.  A board's layout stream may be drawn further
 * ahead than the loop's (refills); the layouts and their order do not differ.
 * Outputs, each of full-batch shape and indexed by board id; only the rows of the boards played
 * are written; reward and done are required, every other pointer may be NULL:
 *   reward      double [B]: r_0, then the sub-steps' rewards added left to right in f64 (TD-atk:
 *               each already negated), as frame skip
 *   done        uint8 [B];  steps_run  int32 [B]: the sub-steps executed
 *   win, allow_next, cooldowns, ep_return, ep_len: what the last executed sub-step would have
 *               written (td_step_io)
 *   first_def   int64 [B], first_atk int64 [B][3][8]: the actions sampled in sub-step 0, byte
 *               for byte td_sample_actions' rows at `ticket` -- which move the playout began with
 * Accounting: the call is one launch for the refill cadence and the ring guard (a board consumes
 * at most one layout per launch) and takes the next td_kernel_timing pair, as the list calls do.
 * It leaves the retained observation behind, as td_copy_boards with obs == NULL: the next step
 * into the retained buffer writes every byte.  td_frame_skip() plays no part and is not changed.
 * Asynchronous on `stream`, which must be the step's stream; nothing is waited for.
 * Refused (< 0, a whole message in td_last_error, nothing enqueued, nothing changed), in this
 * order: a NULL io; a bad size / abi word; a NULL handle; steps outside
 * [1, TD_MAX_PLAYOUT_STEPS]; a missing reward or done; first_def on TD-atk or first_atk on
 * TD-def; a multi-action handle; random_agent = 0.
 * td_playout_boards / td_playout_boards_dev -- the boards a list names, under td_step_boards /
 *   td_step_boards_dev's contracts word for word where they apply.  Host list: n < 0 or n > the
 *   handle's boards, NULL boards with n > 0, an id out of range or named twice are refused on the
 *   host; n == 0 returns 0 and launches nothing; the ids travel through the pinned id slots, so
 *   the caller's array is free on return.  Device list: cap < 0 (with the io words, before the
 *   handle), cap > the handle's boards and NULL boards_dev on the host; cap == 0 returns 0;
 *   TD_LIST_BAD_COUNT, TD_LIST_RANGE, TD_LIST_TWICE on the device (td_list_check_kernel in front,
 *   the next serial of the handle's device-list calls): then no byte of any board, stream or
 *   output changes, the call returned 0 and td_list_errors counts it.  Boards not named keep
 *   every byte of state, both streams, their flags, their staged layouts and their output rows. */
#define TD_MAX_PLAYOUT_STEPS 4096
typedef struct td_playout_io {
  uint32_t size, abi;          /* checked first, as td_step_io / td_sample_io */
  int32_t steps;               /* sub-steps per board, 1 .. TD_MAX_PLAYOUT_STEPS */
  uint32_t def_idle, atk_idle; /* td_sample_io's, in units of 2^-32 */
  uint32_t reserved;           /* 0 */
  uint64_t seed, ticket;       /* td_sample_io's; sub-step j draws at ticket + j */
  double* reward;
  uint8_t* done;
  int32_t* steps_run;
  int8_t* win;
  uint8_t* allow_next;
  uint8_t* cooldowns;
  double* ep_return;
  int32_t* ep_len;
  int64_t* first_def;
  int64_t* first_atk;
} td_playout_io;
/* Zero *io and set its size / abi words. */
void td_playout_io_init(td_playout_io* io);
int td_playout(td_handle* h, const td_playout_io* io, void* stream);
int td_playout_boards(td_handle* h, const td_playout_io* io, const int32_t* boards, int n, void* stream);
int td_playout_boards_dev(td_handle* h, const td_playout_io* io, const int32_t* boards_dev, int cap,
                          const int32_t* count_dev, td_list_status* status_dev, void* stream);
/* The kernel the three calls launch, as rocprofv3 shows it: "td_playout_kernel<10, 0>" (L or 0
 * for a generic side, mode).  The string is the handle's, valid until the next call. */
const char* td_playout_kernel_name(td_handle* h);

/* Probes: `reps` independent random playouts of every board in ONE launch, from the board's
 * present state, which is only read -- what a search does to estimate the value of a state.  No
 * scratch boards, no copy, nothing of the handle changed.  Defined by a call the library already
 * has.  Replica r (0 <= r < reps) of board b is this hypothetical call:
 *   td_playout_boards of board b with the same seed, def_idle, atk_idle and steps, at ticket
 *     ticket + r * steps (mod 2^64), on the board's present state, its effects on the handle
 *     discarded.
 * The replica's reward, done, steps_run, win, first_def and first_atk are that call's outputs.
 * Sub-step j of replica r draws at ticket + r * steps + j; the key is the board id, as in the
 * sampler.  So replica 0 is td_playout_boards at `ticket`, output for output; no two replicas of
 * one call share a ticket; the call takes steps * reps tickets.
 *   Every replica of a board starts from the same position of the board's opponent stream (TD-def,
 *     TD-atk): each runs the built-in opponent on a private copy of the stream's words.  The
 *     replicas differ through the sampled side only; where the sampled side has one legal move
 *     throughout, they are the same playout.
 *   A replica stops after the sub-step that ends its episode.  No reset happens and no staged
 *     layout is consumed; TD_FLAG_NO_LAYOUT is never set; auto-reset on or off makes no difference.
 *   A board never reset gets, for every replica, reward 0, done 1, steps_run 0, win -1, first_def
 *     the no-op and first_atk all 4.  Its header flag is not written.
 * After the call none of these differs from before it: the exported state of any board; either
 * stream, down to the raw MT words, the lazy-twist boundary and the hot record; the flags,
 * td_episode_stats and td_episode_records; the layout rings and their heads; the step count of
 * the refill cadence and the ring guard; the observation buffer and what td_retain_obs knows of
 * it (the next retained step skips as if no probe had run); every output row of td_step and
 * td_playout.  The call may take the next td_kernel_timing pair, and in the device-list form the
 * next list-check serial and a td_list_errors count.  Nothing else of the handle changes.
 * Outputs, each of full-batch shape [B][reps] (first_atk [B][reps][3][8]) and indexed by board
 * id, then replica; only the rows of the boards named are written; reward and done are
 * required, every other pointer may be NULL.
 * Asynchronous on `stream`, which must be the step's stream; nothing is waited for.
 * Refused (< 0, a whole message in td_last_error, nothing enqueued, nothing changed), in this
 * order: a NULL io; a bad size / abi word; a NULL handle; steps outside
 * [1, TD_MAX_PLAYOUT_STEPS]; reps outside [1, TD_MAX_PROBE_REPS]; a missing reward or done;
 * first_def on TD-atk or first_atk on TD-def; a multi-action handle; random_agent = 0.
 * td_frame_skip() plays no part.
 * td_probe_boards / td_probe_boards_dev -- the boards a list names, under td_playout_boards /
 *   td_playout_boards_dev's contracts word for word: a board named twice is refused (replication
 *   is what reps is for), and a refused device list writes nothing. */
#define TD_MAX_PROBE_REPS 256
typedef struct td_probe_io {
  uint32_t size, abi;          /* checked first, as td_playout_io */
  int32_t steps;               /* sub-steps per replica, 1 .. TD_MAX_PLAYOUT_STEPS */
  int32_t reps;                /* replicas per board, 1 .. TD_MAX_PROBE_REPS */
  uint32_t def_idle, atk_idle; /* td_sample_io's, in units of 2^-32 */
  uint64_t seed, ticket;       /* td_sample_io's; sub-step j of replica r draws at ticket + r * steps + j */
  double* reward;              /* [B][reps] */
  uint8_t* done;               /* [B][reps] */
  int32_t* steps_run;          /* [B][reps] */
  int8_t* win;                 /* [B][reps] */
  int64_t* first_def;          /* [B][reps] */
  int64_t* first_atk;          /* [B][reps][3][8] */
} td_probe_io;
/* Zero *io and set its size / abi words. */
void td_probe_io_init(td_probe_io* io);
int td_probe(td_handle* h, const td_probe_io* io, void* stream);
int td_probe_boards(td_handle* h, const td_probe_io* io, const int32_t* boards, int n, void* stream);
int td_probe_boards_dev(td_handle* h, const td_probe_io* io, const int32_t* boards_dev, int cap,
                        const int32_t* count_dev, td_list_status* status_dev, void* stream);
/* The kernel the three calls launch, as rocprofv3 shows it: "td_probe_kernel<10, 0>" (L or 0 for
 * a generic side, mode).  The string is the handle's, valid until the next call. */
const char* td_probe_kernel_name(td_handle* h);

/* Which step kernel td_step launches (one wave per board in all three; they differ in
 * occupancy and load schedule, not in results):
 *   TD_KERNEL_LARGE  td_step_kernel        several rounds of waves (7 per SIMD), live slots
 *                                          loaded once the header's counts are in;
 *   TD_KERNEL_SMALL  td_step_kernel_small  one round (8 waves per SIMD), 16 enemy + 16 tower
 *                                          slots prefetched with the header;
 *   TD_KERNEL_SMALL2 td_step_kernel_small2 as SMALL, plus a second wave per board that
 *                                          writes half of the observation;
 *   TD_KERNEL_AUTO   td_create's rule: SMALL2 up to half a round of boards, SMALL up to one
 *                    round, SMALL2 again above that -- at any batch for single-action TD-def
 *                    at L = 10, up to 3 rounds for the other L = 10 modes, 10 rounds at
 *                    L = 30 (single-action) and 8 rounds for TD-2p multi-action at L = 20 --
 *                    else LARGE (L = 10 / 20 / 30; other L only have LARGE).  With
 *                    TD_OBS_F16 at L = 10: SMALL2 up to half a round, SMALL above.
 * The kernel is chosen per launch.  The rule above is the kind of a launch that writes every
 * window of the observation: every td_step of a handle that retains nothing, and with
 * td_retain_obs the first step and any step after the buffer stopped being known (the list
 * above td_retain_obs).  Such a launch is bound by its stores.  A skipping launch -- a td_step
 * into the retained buffer that leaves clean windows unwritten -- stores less than half the
 * bytes and is bound by the boards in flight, so TD_KERNEL_AUTO resolves a second kind for it:
 * the first kind, except where a kernel with more boards in flight measured faster --
 * float32, L = 10, single-action TD-def above one round of boards: SMALL where the first kind
 * is SMALL2 (DESIGN.md section 4 has the measurements).  Both kinds see the same board state
 * and give the same results, so the hand-over between them needs nothing.
 * The small kernels need a 16-B-aligned observation buffer (8-B-aligned with TD_OBS_F16);
 * a td_step with any other buffer runs LARGE.  (Forcing a kind is a test hook: td_set_step_kernel, td_diag.h;
 * a kind forced there is forced for every launch.)
 * td_step_kernel returns the resolved kind of a launch that writes every window,
 * td_retained_step_kernel that of a skipping launch.  td_step_kernel_name is the
 * kernel's name as rocprofv3 shows it ("td_step_kernel_small<10, 0, false>": L, mode,
 * multi-action scan): the kernel the most recent td_step launched; before the first td_step,
 * and after a change of kernel, format or frame skip, the kernel of a launch that writes every
 * window.  The string is the handle's, valid until the next call. */
enum td_step_kernel_kind { TD_KERNEL_AUTO = 0, TD_KERNEL_LARGE = 1, TD_KERNEL_SMALL = 2, TD_KERNEL_SMALL2 = 3 };
int td_step_kernel(td_handle* h);
int td_retained_step_kernel(td_handle* h);
const char* td_step_kernel_name(td_handle* h);
/* The kernel td_step_boards launches on this handle, as rocprofv3 shows it:
 * "td_step_sel_kernel<10, 0, false>" (L or 0 for a generic side, mode, multi-action scan), or
 * "td_step_sel_kernel_f16<...>" with TD_OBS_F16: one wave per named board in TD_KERNEL_LARGE's
 * shape, whatever kind td_step launches.  The string is the handle's, valid until the next call. */
const char* td_step_boards_kernel_name(td_handle* h);
/* The kernel td_step_boards_dev launches behind its check kernel: "td_step_list_kernel<10, 0,
 * false>" or "td_step_list_kernel_f16<...>", the same rows and shape as td_step_boards'.  The
 * string is the handle's, valid until the next call. */
const char* td_step_boards_dev_kernel_name(td_handle* h);

/* Steps between launches of the layout refill kernel on the side streams (auto-reset;
 * default 64, 0 = none).  A pure performance knob: before every 15th step (and the first
 * step after a reset) the ring guard runs on the step stream and brings every board's
 * ring of 16 staged layouts to at least 15, so an episode end always finds its next
 * layout, whatever the interval.  The only board that misses one is a board whose draws
 * fail 65 times in a row (where the reference raises): it is flagged no_layout. */
int td_set_refill_interval(td_handle* h, int steps);

/* Kernel timing: every `every`-th td_step call from now on, up to max_launches of them,
 * binds a pair of timing events to its step kernel's own dispatch (hipExtLaunchKernel;
 * no marker packets); max_launches = 0 turns it off.  td_kernel_times waits for them
 * and writes each kernel's start-to-end duration in microseconds (the dispatch-packet
 * timestamps rocprofv3 reports); returns the count.  A td_copy_boards call made while pairs
 * are left takes the next pair for its copy kernel as well, whatever `every` is. */
int td_kernel_timing(td_handle* h, int max_launches, int every);
int td_kernel_times(td_handle* h, float* us, int cap);

/* Episodes finished by td_step since the last clear (SURVEY.md §8(b) td_episode_stats):
 * dev_out[0] = count, dev_out[1] = sum of their returns (f64, device memory, asynchronous
 * on `stream`; the sum is accumulated with atomics, so its rounding order is unspecified).
 * clear != 0 zeroes the accumulators after the copy.  The per-rank values are what the
 * multi-GPU driver gathers over RCCL. */
int td_episode_stats(td_handle* h, double* dev_out, int clear, void* stream);

/* Each board's last finished episode, the per-episode record a trainer collects
 * (train/main.py:155-166: total reward, length, win): dev_out = B records of 16 bytes,
 * { f64 return; i32 length; i32 win (1, 0, or -1 before the first finished episode) },
 * device memory, asynchronous on `stream`.  SURVEY.md §8(e): the per-board payload the
 * multi-GPU driver gathers over RCCL once per reporting interval. */
typedef struct td_episode_record {
  double ret;
  int32_t length;
  int32_t win;
} td_episode_record;
int td_episode_records(td_handle* h, td_episode_record* dev_out, void* stream);

/* The built-in opponent acting on its own between steps, as TDGymBasic's methods do when
 * called directly (TDGymBasic.py:81-108 random_enemy_lv0/1, :111-292 random_tower_lv0/1/2;
 * demo.py:78-79): side 0 = random_enemy_lv<level>, side 1 = random_tower_lv<level>, for the
 * boards in host_mask (NULL = all), on each board's opponent stream, with the reference's
 * cool-down check and update.  Synchronous. */
int td_opponent(td_handle* h, int side, int level, const uint8_t* host_mask, void* stream);

/* Layout records.
 * td_layout_from_roads: road i is cells[offsets[i] .. offsets[i + 1]) (row * L + col, start
 * first), stamped in order as TDBoard.__init__ stamps its map planes; a later road overwrites
 * the direction and distance of the cells it shares with an earlier one, and max dist is the
 * maximum of the finished distance plane (TDBoard.py:121-122).
 * The layout rule: every road is a simple 4-connected path of 2 .. 64 cells, and every road
 * leads into road 0's last cell (the end cell).  Returns non-zero, with rec[0] = 0 (not a
 * record), for num_roads outside 1 .. 3, an empty road, a cell outside the board, a road of
 * more than 64 cells (the step kernels normalise the distance plane through a 64-entry
 * table; create_road_v2 draws at most 2 L - 1 <= 63 cells) and a road that names a cell twice
 * (such a loop can never be walked: the second exit's direction overwrites the first).
 * Connectivity and the common end are the caller's: a road that dead-ends elsewhere is stepped
 * under the TD_FLAG_BAD_MOVE rule (td_board_flag). */
int td_layout_words(int map_size);
int td_layout_from_roads(int map_size, int num_roads, const int32_t* cells, const int32_t* offsets, uint32_t* rec);
/* TDGymBasic.reset's draws on one numpy-legacy stream: num_roads = randint(1, 4),
 * then create_road_v2.  Returns 0 or a road-generation error code (>0). */
int td_layout_generate(uint32_t* np_state625, int map_size, int max_attempts, uint32_t* rec);

/* Board state, array-major for boards [b0, b0+count):
 *   hdr[count] (96 B each: see td_common.h TdHdr), en_lp f64[count][128], en_mg f64[count][128],
 *   en_inf u32[count][128] (cell | type<<12 | lv<<14 | slowdown<<16 | config epoch<<24),
 *   tw_cd f64[count][32], tw_inf u32[count][32] (cell | type<<12 | lv<<14 | build epoch<<16 |
 *   stats epoch<<24; imported entities take the current epoch), cells u32[count][L*L],
 *   opp_mt u32[count][626] (the opponent's CPython stream: 624 words, position, and the
 *   lazy-twist boundary -- words [w[625], 624) still hold the previous block).  Synchronous.
 *   The board's numpy layout stream is not part of the record (it belongs to the stream of
 *   layouts, staged ahead under auto-reset): save / restore it with td_get_np_state /
 *   td_set_np_state -- with random_agent=False it is also the built-in opponent's stream.
 *   td_import_state checks the header of every board that has a layout (format, captured
 *   max_cost / max_base_LP, list counts, max dist in 0 .. 63) before it copies anything; a
 *   refused record leaves nothing imported. */
size_t td_state_bytes(td_handle* h, int count);
int td_export_state(td_handle* h, int b0, int count, void* host_dst);
int td_import_state(td_handle* h, int b0, int count, const void* host_src);
int td_get_flags(td_handle* h, int32_t* host_flags);

/* Ring-guard waits for a board's refill claim that gave up after 1 s (a claim never given
 * back): the board is flagged TD_FLAG_CLAIM_TIMEOUT and its ring may run short.  Returns the
 * count since the last clear (clear != 0 zeroes it).  Synchronous. */
int td_guard_timeouts(td_handle* h, int clear);

/* Host-side RNG helpers (exposed for tests and for seeding from Python states). */
void td_py_seed(uint32_t* mt625, uint32_t seed);
void td_np_seed(uint32_t* mt625, uint32_t seed);
uint32_t td_mt_next(uint32_t* mt625);
int64_t td_py_randint(uint32_t* mt625, int64_t a, int64_t b);
int64_t td_np_randint(uint32_t* mt625, int64_t lo, int64_t hi);

#ifdef __cplusplus
}
#endif
#endif /* TDSTEP_H_ */
