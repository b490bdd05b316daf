// td_step_small2.inc -- the two-wave step kernel, included by td_step.hip and td_step_f16.hip,
// once per observation format, with TD_SMALL2_NAME (the kernel) and TD_SMALL2_OT (the output element)
// defined.  One text instead of a function template both kernels call: the float32 kernel,
// the one bench.py measures, stays the kernel it was, instruction for instruction (a shared
// body function compiled to different code).
template <int LT, int MODE, bool SCAN>
__global__ __launch_bounds__(128) TD_SMALL2_ATTR void TD_SMALL2_NAME(StepArgs a_) {
  const StepArgs& a = kargs(a_);
  constexpr int NC = LT * LT;
  __shared__ Smem<NC> S;
  __shared__ StepOut SO;
  prologue_args(a);
  if ((int)blockIdx.x >= a.B) return;
  const int b = a.xcd_map ? xcd_board((int)blockIdx.x, a.B) : (int)blockIdx.x;
  const int lane = (int)threadIdx.x & 63;
  if (threadIdx.x < 64) {
    const Ctx x{S.cfg, LT, NC, lane, a.cfgs, a.epoch, side_magic(LT), false};
    const uint4 cfgv = load_cfg(a.cfg, lane);
    Prefetch P;
    prefetch_issue<PF_SMALL, PF_SMALL>(P, a, b, lane, NC, MODE != MODE_ATK && !a.multi);
    store_cfg(S, cfgv, lane);  // (see load_cfg)
    wsync();  // every lane reads the block: no LDS access may move above its store
    step_board<NC, LT, MODE, SCAN, true, true, TD_SMALL2_OT>(S, x, a, b, P, &SO);
  } else {
    typedef TD_SMALL2_OT OT;
    OT* const obs = reinterpret_cast<OT*>(a.obs) + (size_t)b * NCH * NC;
    constexpr bool SCAN2 = SCAN;
    if constexpr (SCAN2) {  // the multi-action flags, folded while the first wave loads the board
      const bool bad = scan_fold(S, lane, NC, a.def_act + (size_t)b * 6 * NC);
      if (lane == 0) SO.scan_bad = bad ? 1u : 0u;
      __syncthreads();  // (A0)
    }
    __syncthreads();  // (A) actions and towers final, cells packed
    if constexpr (SCAN2) {  // the real actions, beside the step (grp[1] is not touched before (B))
      if (S.early_go && a.real_def) scan_write_real(S, lane, NC, a.real_def + (size_t)b * 6 * NC);
    }
    if (const uint32_t early = S.early_go & OD_ALL) {  // (kEarlyGo alone: no binary-plane window is dirty)
      if (early == OD_ALL) write_obs_lines<NC, LT, 0, -1, 4, 1, OT>(S, lane, obs, false, a.obs_wt != 0, a.edge_wt);
      else write_obs_lines<NC, LT, 0, -1, 4, 1, OT, true>(S, lane, obs, false, a.obs_wt != 0, a.edge_wt, early);
      // landed before (B): after an auto-reset the first wave rewrites these windows
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();  // (B) the board after the step and its outputs are in SO
    const uint32_t go = SO.go;
    if (go) {
      static_assert(sizeof(TdHdr) == 6 * 16 && offsetof(StepOut, hdr) == 0 && alignof(StepOut) >= 16,
                    "header copied as 6 x 16-B LDS reads");
      if (lane < (SO.hdr_hi ? 6 : 3)) reinterpret_cast<uint4*>(a.hdr + b)[lane] = reinterpret_cast<const uint4*>(&SO.hdr)[lane];
      store_towers(S, SO.nt, SO.tw_dirty != 0, lane, a, b);
      store_outputs(a, b, SO, lane);
    }
    __syncthreads();  // (C) statistics and broadcast channels in LDS
    if (go == 1u) {
      if (SO.dirty == OD_ALL)
        write_obs_lines<NC, LT, obs_late_half<LT, OT>(), -1, 4, 2, OT>(S, lane, obs, SO.any != 0u, a.obs_wt != 0, a.edge_wt);
      else
        write_obs_lines<NC, LT, obs_late_half<LT, OT>(), -1, 4, 2, OT, true>(S, lane, obs, SO.any != 0u, a.obs_wt != 0,
                                                                            a.edge_wt, SO.dirty);
    }
  }
}
