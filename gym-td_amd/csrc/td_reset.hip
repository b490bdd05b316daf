// td_reset.hip -- the kernels that run between steps: td_opponent_kernel (a built-in opponent
// called on its own), one wave's layout draw (wave_layout) with the reset, auto-reset and refill
// kernels that use it, td_cfg_usage_kernel, and the launchers of all five.  None is on a step's
// critical path, and each serves both observation formats (reset_one branches on a.obs_f16).
#include "td_kernels.h"
#include "td_layout.h"
#include "td_step_launch.h"
#include "td_step_obs.h"
#include "td_step_opp.h"
#include "td_step_state.h"
#include "td_wavegen.h"

namespace td {

// The built-in opponents called on their own, between steps (TDGymBasic.py:81-292,
// called directly by demo.py:78-79): random_enemy_lv{0,1} (side 0) or
// random_tower_lv{0,1,2} (side 1) for every masked board, on the board's opponent
// stream, with the reference's cool-down check and update.  No observation.
template <int LT>
__global__ __launch_bounds__(64) void td_opponent_kernel(StepArgs a, int side, int level) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ Smem<NC> S;
  const int b = blockIdx.x;
  if (b >= a.B) return;
  if (a.reset_mask && !a.reset_mask[b]) return;
  stage_cfg(S, a.cfg);
  const int L = LT ? LT : a.L;
  const Ctx x{S.cfg, L, L * L, (int)threadIdx.x, a.cfgs, a.epoch};
  Prefetch P;
  prefetch_issue<PF_SMALL, PF_SMALL>(P, a, b, x.lane, x.NCr, false);
  U u;
  load_board<NC, PF_SMALL, PF_SMALL>(S, u, x, a, b, P);
  if (u.num_roads < 1 || u.num_roads > 3) return;  // never reset: nothing to act on
  uint32_t* const hot = a.opp_hot + (size_t)b * HOT_WORDS;
  WaveMt R{a.opp_mt + (size_t)b * OPP_WORDS, lane_word(P.w, PF_HOT + 0), lane_word(P.w, PF_HOT + 1)};
  R.cn = lane_word(P.w, PF_HOT + 2);
  R.cbase = lane_word(P.w, PF_HOT + 3);
  R.cache = __shfl(P.w, PF_HOT + 4 + (x.lane < HOT_CACHE ? x.lane : 0));
  with_opp_rng(a, b, x.lane, R, [&](auto& G) {
    if (side == 0) opponent_enemy(S, u, x, G, level);
    else opponent_tower(S, u, x, G, level);
  });
  __syncthreads();
  R.prefetch(x.lane);  // the next step expects the hot record primed
  const size_t eb = (size_t)b * ECAP;
  for (int i = x.lane; i < u.n; i += 64) {
    sst(&a.en_lp[eb + i], S.eLP[i]);
    sst(&a.en_mg[eb + i], S.eMg[i]);
    sst(&a.en_inf[eb + i], S.eInf[i]);
  }
  store_cells(S, u, x, a, b);
  store_board(S, u, x, a, b);
  if (x.lane == 0) { hot[0] = R.pos; hot[1] = R.tw; hot[2] = R.cn; hot[3] = R.cbase; }
  if (x.lane < HOT_CACHE) hot[4 + x.lane] = R.cache;
}

// Layout draws are resumable (RoadGen::draw): a refill gives each board a budget of
// walks per launch, and a draw that runs out (in practice one the reference never
// finishes, ~1,000 walks per retry loop) keeps its state in the board's HBM scratch
// -- the RoadResume header, then the generator's arrays -- with the partial record
// in the ring slot (its tag still the old one) and the stream position in np_mt.
// The next refill continues it draw for draw.  So a refill launch runs at most
// ~a.refill_walks walks per board -- except for a board whose ring is empty, whose
// draw runs to the end at once (rare: the initial fill, or episodes shorter than the
// refill can follow).
__device__ __forceinline__ RoadResume* resume_hdr(const StepArgs& a, int b) {
  return reinterpret_cast<RoadResume*>(a.scratch + (size_t)b * a.scratch_stride);
}

// TDGymBasic.reset's draws (:42-51) for board b into slot `slot` of its ring, as
// layout number `n` of the stream: failing draws are skipped up to ``retries``
// times, at most ``budget`` walks are run (ROAD_PENDING: continued by a later call).
// A finished record is published for a step grid that may be running on another
// stream: plain stores, every lane's vmcnt(0), the barrier, ONE agent-scope
// release, then the tag by an sc1 store (MI355X_MICROARCH.md § visibility, "Valid
// forms", producer bullet).  Returns the road status of the last draw.
template <int NC, bool SBP = false>
__device__ int wave_layout(LayoutSmem<NC>& G, const StepArgs& a, int b, int retries, uint32_t* slot, uint32_t n,
                           int budget) {
  const int lane = (int)threadIdx.x, L = a.L, lw = LAYOUT_HDR + L * L;
  const int sbytes = (int)road_scratch_bytes(L);
  // (the walk budget and the retry count bound the draw's loop: wave-uniform, SGPRs)
  budget = (int)__builtin_amdgcn_readfirstlane((uint32_t)budget);
  retries = (int)__builtin_amdgcn_readfirstlane((uint32_t)retries);
  uint32_t* gmt = a.np_mt + (size_t)b * OPP_WORDS;
  RoadResume* ghdr = resume_hdr(a, b);
  uint8_t* gscr = a.scratch + (size_t)b * a.scratch_stride + sizeof(RoadResume);
  for (int i = lane; i < OPP_WORDS; i += 64) G.mt[i] = gmt[i];
  if (lane < 16) reinterpret_cast<uint32_t*>(&G.res)[lane] = reinterpret_cast<const uint32_t*>(ghdr)[lane];
  __syncthreads();
  const bool resumed = G.res.phase != RP_NEW;  // wave-uniform
  if (resumed) {
    for (int i = lane; i < sbytes / 4; i += 64) reinterpret_cast<uint32_t*>(G.scratch)[i] = reinterpret_cast<const uint32_t*>(gscr)[i];
    for (int i = 1 + lane; i < lw; i += 64) G.rec[i] = slot[i];
    __syncthreads();
  }
  int st = ROAD_ERR_BOUND;
  {
    WaveRoadGen<NC, SBP> g;
    g.carve(G.scratch, L * L);
    g.mt = G.mt; g.rec = G.rec; g.L = L; g.lane = lane;
    // the stream position and the resume state are wave-uniform: SGPRs
    g.pos = __builtin_amdgcn_readfirstlane(G.mt[MT_N]);
    g.tw = __builtin_amdgcn_readfirstlane(G.mt[MT_N + 1]);
    g.base = g.pos; g.n = 0; g.win = 0;
    RoadResume res;
    for (int i = 0; i < 16; ++i)
      reinterpret_cast<uint32_t*>(&res)[i] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t*>(&G.res)[i]);
    g.load_maps(resumed);  // the draw's field / turn bitmaps
    st = g.draw(res, budget, kRoadAttempts, retries);
    __syncthreads();
    g.save_maps();
    if (lane == 0) { G.mt[MT_N] = g.pos; G.mt[MT_N + 1] = g.tw; G.res = res; }
  }
  __syncthreads();
  // every store below is write-through (st_relaxed = sc1): the claim release and the
  // tag store publish them without a release fence (see claim_board)
  for (int i = lane; i < OPP_WORDS; i += 64) st_relaxed(gmt + i, G.mt[i]);
  if (lane < 16) st_relaxed(reinterpret_cast<uint32_t*>(ghdr) + lane, reinterpret_cast<const uint32_t*>(&G.res)[lane]);
  if (st == ROAD_PENDING) {  // keep the draw for the next call (published by the caller's claim release)
    for (int i = lane; i < sbytes / 4; i += 64)
      st_relaxed(reinterpret_cast<uint32_t*>(gscr) + i, reinterpret_cast<const uint32_t*>(G.scratch)[i]);
    for (int i = 1 + lane; i < lw; i += 64) st_relaxed(slot + i, G.rec[i]);
  } else if (st == ROAD_OK) {
    for (int i = 1 + lane; i < lw; i += 64) st_relaxed(slot + i, G.rec[i]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every lane's record stores have landed
    __syncthreads();
    if (lane == 0) st_relaxed(slot, slot_tag(n));
  }
  return st;
}

// TDGymBasic.reset of board b, by one wave (the device is idle for this board: no refill
// holds it).  The layout is the caller's record (td_reset_layouts), else the board's
// next staged layout, else a draw from its numpy stream now -- skipping up to `retries`
// failing draws.  A draw that still fails leaves the board unchanged and returns its
// road status (the reference raises); else the board is reset, its first observation
// written, and ROAD_OK returned.  keep_flags: an auto-reset keeps the board's flags,
// an explicit reset clears them.
template <int NC, int LT>
__device__ int reset_one(Smem<NC>& S, LayoutSmem<NC>& gen, const StepArgs& a, int b, int retries, bool keep_flags) {
  const int L = LT ? LT : a.L;
  const uint32_t* rec;
  bool from_ring = false;
  uint32_t head = 0;
  const int ov = a.ovr_idx ? a.ovr_idx[b] : -1;
  if (ov >= 0) {
    rec = a.ovr_rec + (size_t)ov * (LAYOUT_HDR + L * L);
  } else {
    head = a.lay_head[b];
    const uint32_t tail = a.lay_tail[b];
    uint32_t* slot = a.nxt + ((size_t)b * NSLOT + head % NSLOT) * a.slot_words;
    if (tail == head) {  // nothing staged: draw now
      const int st = wave_layout(gen, a, b, retries, slot, head, 0x7fffffff);
      __syncthreads();
      if (st != ROAD_OK) return st;
      if (threadIdx.x == 0) a.lay_tail[b] = tail + 1u;
    }
    rec = slot;
    from_ring = true;
  }
  stage_cfg(S, a.cfg);
  __syncthreads();
  const Ctx x{S.cfg, L, L * L, (int)threadIdx.x, a.cfgs, a.epoch};
  U u;
  u.episodes = a.hdr[b].episodes;
  u.flags = keep_flags ? a.hdr[b].flags : 0;
  reset_board(S, u, x, rec);
  channel_scalars(S, u, x);
  store_cells(S, u, x, a, b);
  pack_obs_cells(S, x);
  if (a.obs) {  // (the format a run-time branch here: a reset is no hot path, and its kernels keep one build)
    if (a.obs_f16) reset_obs<NC, LT, _Float16>(S, x, a, b);
    else reset_obs<NC, LT, float>(S, x, a, b);
  }
  store_board(S, u, x, a, b);
  if (x.lane == 0 && from_ring) a.lay_head[b] = head + 1u;
  return ROAD_OK;
}

template <int NC>
union ResetSmem {
  Smem<NC> board;
  LayoutSmem<NC> gen;
};

// TDGymBasic.reset for the boards in reset_mask (td_reset / td_reset_layouts: the
// device is idle, td_capi synchronises first).  A failing draw (no retry) is reported
// in reset_fail and leaves the board unchanged, as the reference raises.
template <int LT>
__global__ __launch_bounds__(64) void td_reset_kernel(StepArgs a) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ ResetSmem<NC> sh;
  const int b = blockIdx.x;
  if (b >= a.B) return;
  if (a.reset_mask && !a.reset_mask[b]) return;
  const int st = reset_one<NC, LT>(sh.board, sh.gen, a, b, 0, false);
  if (threadIdx.x == 0) a.reset_fail[b] = (uint8_t)st;
}

// Auto-reset with random_agent=False (TDGymBasic.py:87-89,101-103 under gym 0.21's
// AsyncVectorEnv, which calls reset() right after the step that ends an episode): the
// built-in opponent and reset() draw from the same numpy stream, so the next layout
// cannot be drawn ahead of play.  Launched right behind each step kernel on its
// stream: a wave scans 64 boards' done flags (written by that step) and resets the
// finished boards in turn, drawing each layout from the board's stream now, exactly
// where the reference's reset() would -- failing draws skipped as in every auto-reset.
// The step kernel left those boards finished (no staged layout is consumed in this
// mode); their observation is overwritten with the new episode's first one.  Boards
// flagged FLAG_NO_LAYOUT are skipped: a board never reset (its first road generation
// failed, done every step) or whose auto-reset already failed 65 draws in a row stays
// as it is until an explicit reset, as under random_agent=True -- it neither stalls
// the step stream with 65 draws every step nor consumes its stream.
template <int LT>
__global__ __launch_bounds__(64) void td_autoreset_kernel(StepArgs a) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ ResetSmem<NC> sh;
  const int lane = (int)threadIdx.x;
  const int b0 = (int)blockIdx.x * 64;
  const bool mine = b0 + lane < a.B && a.done[b0 + lane] != 0 && !(a.hdr[b0 + lane].flags & FLAG_NO_LAYOUT);
  uint64_t m = ballot(mine);
  while (m) {
    const int b = b0 + ctz64(m);
    m &= m - 1;
    const int st = reset_one<NC, LT>(sh.board, sh.gen, a, b, kLayoutRetries, true);
    __syncthreads();
    if (st != ROAD_OK && lane == 0) a.hdr[b].flags |= FLAG_NO_LAYOUT;  // keeps stepping its finished episode
  }
}

// Keep every board's ring of staged layouts full: lanes check G boards at once
// (layouts drawn minus consumed < NSLOT), then the wave draws the missing layouts
// of those boards one by one with the whole-wave generator (WaveRoadGen).
//
// guard = 0 (refill): runs on a side stream concurrently with the step grids, which
// never wait for it; a board another refill holds is skipped, and a draw gets at most
// a.refill_walks walks unless the ring is empty.
//
// guard = G > 0 (ring guard): runs ON the step stream, between two steps, before every
// G-th step (td_capi.hip td_step): every ring holding fewer than G complete layouts is
// filled to G -- draws run to the end, a board a side refill holds is waited for (its
// wave is resident and gives the claim back after its walk budget).  A board consumes
// at most one layout per step, so none of the next G steps finds its ring empty: an
// episode end never depends on the refill cadence (TDGymBasic.py:37-55 resets at every
// end).  The one exception is the reference's own failure, 65 failing draws in a row
// (it raises): the ring stays short and the step flags the board no_layout.  Rings
// below G are rare when the side refills keep up (a board would have to finish
// NSLOT - G + 1 episodes between two refills), so a guard launch is mostly a scan.
template <int LT>
__global__ __launch_bounds__(64) void td_refill_kernel(StepArgs a, int guard) {
  constexpr int NC = LT ? LT * LT : MAX_KERNEL_L * MAX_KERNEL_L;
  __shared__ LayoutSmem<NC> G;
  const int lane = (int)threadIdx.x;
  const int grp = a.refill_grp;
  const uint32_t level = guard ? (uint32_t)guard : (uint32_t)NSLOT;  // layouts wanted per ring
  for (int base = (int)blockIdx.x * grp; base < a.B; base += (int)gridDim.x * grp) {
    const int b = base + lane;
    const bool mine = lane < grp && b < a.B;
    uint32_t head = 0, tail = 0;
    if (mine) {
      head = ld_relaxed(a.lay_head + b);  // a step grid may be advancing it right now
      tail = ld_relaxed(a.lay_tail + b);
    }
    uint64_t m = ballot(mine && tail - head < level);
    while (m) {
      const int l = ctz64(m);
      m &= m - 1;
      const int bb = base + l;
      if (!claim_board(a.lay_claim + bb, lane)) {  // another refill is drawing its layouts
        if (!guard) continue;
        // a board whose claim wait already gave up is not waited for again (a claim never
        // given back would stall every guard launch 1 s); it is not counted twice either
        if (ld_relaxed((const uint32_t*)&a.hdr[bb].flags) & FLAG_CLAIM_TIMEOUT) continue;
        // the holder is a resident side-refill wave that gives the claim back after its
        // walk budget; bounded all the same (1 s, as take_dry_ring): a claim never given
        // back leaves this board's ring short -- its episode end is then flagged
        // no_layout by the step -- instead of hanging the step stream
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        bool got = false;
        while (!got && __builtin_amdgcn_s_memrealtime() - t0 < kTakeSpinTicks) {
          __builtin_amdgcn_s_sleep(8);
          got = claim_board(a.lay_claim + bb, lane);
        }
        if (!got) {  // visible: the board's flag and the engine's counter (td_guard_timeouts)
          if (lane == 0) {
            atomicOr(&a.hdr[bb].flags, FLAG_CLAIM_TIMEOUT);
            if (a.guard_to) atomicAdd(a.guard_to, 1u);
          }
          continue;
        }
      }
      uint32_t t = __builtin_amdgcn_readfirstlane(ld_relaxed(a.lay_tail + bb));  // (wave-uniform: SGPRs)
      const uint32_t h = __builtin_amdgcn_readfirstlane(ld_relaxed(a.lay_head + bb));
#pragma nounroll
      while (t - h < level) {
        uint32_t* slot = a.nxt + ((size_t)bb * NSLOT + t % NSLOT) * a.slot_words;
        // an empty ring is urgent (the board needs this layout at its next episode end):
        // its draw runs to the end; otherwise at most a.refill_walks walks this launch
        const int st = wave_layout<NC, kGenSBProof && NC <= 128>(
            G, a, bb, kLayoutRetries, slot, t, t == h || guard ? 0x7fffffff : a.refill_walks);
        __syncthreads();
        if (st != ROAD_OK) break;  // out of walks (continued next launch), or 65 failing draws in a row
        ++t;
      }
      if (lane == 0) st_relaxed(a.lay_tail + bb, t);
      release_board(a.lay_claim + bb, lane);
    }
  }
}

// The paramConfig epochs live enemies and towers still refer to (td_set_config
// recycles the others): one wave per board, bits OR-ed into used[NCFG / 32].
__global__ __launch_bounds__(64) void td_cfg_usage_kernel(StepArgs a, uint32_t* used) {
  const int b = blockIdx.x, l = (int)threadIdx.x;
  if (b >= a.B) return;
  const int n = a.hdr[b].n_en, nt = a.hdr[b].n_tw;
  for (int i = l; i < n; i += 64) {
    const int e = en_ep(a.en_inf[(size_t)b * ECAP + i]);
    atomicOr(&used[e >> 5], 1u << (e & 31));
  }
  if (l < nt) {
    const uint32_t ti = a.tw_inf[(size_t)b * TCAP + l];
    atomicOr(&used[tw_ec(ti) >> 5], 1u << (tw_ec(ti) & 31));
    atomicOr(&used[tw_eu(ti) >> 5], 1u << (tw_eu(ti) & 31));
  }
}

hipError_t launch_opponent(const StepArgs& a, int side, int level, hipStream_t s) {
  with_side(a.L, [&](auto lt) {
    hipLaunchKernelGGL(td_opponent_kernel<decltype(lt)::value>, dim3(a.B), dim3(64), 0, s, a, side, level);
  });
  return hipGetLastError();
}
hipError_t launch_reset(const StepArgs& a, hipStream_t s) {
  with_side(a.L, [&](auto lt) { hipLaunchKernelGGL(td_reset_kernel<decltype(lt)::value>, dim3(a.B), dim3(64), 0, s, a); });
  return hipGetLastError();
}
hipError_t launch_autoreset(const StepArgs& a, hipStream_t s) {
  with_side(a.L, [&](auto lt) {
    hipLaunchKernelGGL(td_autoreset_kernel<decltype(lt)::value>, dim3((a.B + 63) / 64), dim3(64), 0, s, a);
  });
  return hipGetLastError();
}
hipError_t launch_refill(const StepArgs& a_, hipStream_t s, int guard) {
  StepArgs a = a_;
  if (guard) a.refill_grp = 64;  // the guard mostly scans: one ballot of 64 boards per wave, one wave per 64 boards
  const int grp = a.refill_grp;
  const int groups = (a.B + grp - 1) / grp;  // a wave walks the groups grid-stride
  const int waves = guard || groups < a.refill_waves ? groups : a.refill_waves;
  with_side(a.L, [&](auto lt) {
    hipLaunchKernelGGL(td_refill_kernel<decltype(lt)::value>, dim3(waves), dim3(64), 0, s, a, guard);
  });
  return hipGetLastError();
}
hipError_t launch_cfg_usage(const StepArgs& a, uint32_t* used, hipStream_t s) {
  hipLaunchKernelGGL(td_cfg_usage_kernel, dim3(a.B), dim3(64), 0, s, a, used);
  return hipGetLastError();
}

}  // namespace td
