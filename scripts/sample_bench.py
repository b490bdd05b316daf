#!/usr/bin/env python
"""Time of the legal-action sampler (td_sample_actions) beside the mask kernel and beside the
path a caller had before it.  Needs a GPU; not part of bench.py's metric.

    python scripts/sample_bench.py [--launches 50] [--warmup 10] [--burnin 64] [--shape NAME]

Per shape, in one process of its own (without --shape the script starts one child per shape,
one after the other), on boards ``--burnin`` steps into a rollout, three things are timed with
a device-event pair around each of ``--launches`` launches after ``--warmup`` warm-up launches:

  sample      TDEngine.sample_actions()                          one td_sample_kernel
  mask        TDEngine.action_mask()                             one td_mask_kernel: the yardstick
  mask+torch  action_mask() + torch.multinomial(mask.float(), 1) what a caller did before
              (both sides in TD-2p; multi-action rows get a column of ones appended, since a
              row without a legal flag is no distribution)

The three are measured in rounds of one launch each, alternating, so a drift of the machine
meets all three alike.  The event pair brackets one call on an idle stream, so each figure
includes the call's own start-up, the same for all three.  Shapes: 65,536 x 10x10 TD-def,
4,096 x 10x10 TD-def, 16,384 x 30x30 TD-def (burn-in: scripts/mask_bench.py's random-action
rollout) and 16,384 x 20x20 TD-2p multi-action (burn-in: the sampler itself, idle 0.3).
One JSON line per shape: microseconds per call (median, min, mean) of each, and the sampler's
median over the mask's.  There is no pass mark."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))

SHAPES = {
    "def10x65536": (10, 65536, "def", False),
    "def10x4096": (10, 4096, "def", False),
    "def30x16384": (30, 16384, "def", False),
    "2pmulti20x16384": (20, 16384, "2p", True),
}


def make(L, B, mode, multi, burnin):
    from gym_TD.engine import TDEngine
    seeds = np.arange(B)
    eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False)
    eng.reset_all()
    if mode == "def" and not multi:
        g = torch.Generator(device=eng.device)
        g.manual_seed(1)
        acts = torch.randint(0, 6 * L * L + 1, (burnin, B), generator=g, device=eng.device, dtype=torch.int64)
        for k in range(burnin):
            eng.step(def_act=acts[k])
    else:
        for k in range(burnin):
            out = eng.sample_actions(ticket=k, def_idle=0.3, atk_idle=0.3)
            eng.step(def_act=out["def"], atk_act=out["atk"])
    torch.cuda.synchronize()
    return eng


def one_shape(name, args):
    L, B, mode, multi = SHAPES[name]
    eng = make(L, B, mode, multi, args.burnin)
    ones = torch.ones((B, 1), dtype=torch.float32, device=eng.device)

    def sample():
        eng.sample_actions()

    def mask():
        eng.action_mask()

    def mask_torch():
        m = eng.action_mask()
        if "def" in m:
            p = m["def"].reshape(B, -1).float()
            torch.multinomial(torch.cat([p, ones], dim=1) if multi else p, 1)
        if "atk" in m:
            torch.multinomial(m["atk"].reshape(B, -1).float(), 1)

    calls = {"sample": sample, "mask": mask, "mask+torch": mask_torch}
    try:
        for _ in range(args.warmup):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(args.launches):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3)
        out = {"what": "sampler beside the mask", "shape": name, "L": L, "boards": B, "mode": mode, "multi": multi,
               "launches": args.launches, "kernel": eng.sample_actions_kernel_name()}
        for k, v in us.items():
            out[k] = {"us_median": round(float(np.median(v)), 2), "us_min": round(float(np.min(v)), 2),
                      "us_mean": round(float(np.mean(v)), 2)}
        out["sample_over_mask"] = round(out["sample"]["us_median"] / out["mask"]["us_median"], 3)
        out["mask+torch_over_sample"] = round(out["mask+torch"]["us_median"] / out["sample"]["us_median"], 2)
        print(json.dumps(out), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    args = ap.parse_args()
    if args.shape is None:  # one fresh process per shape
        for name in SHAPES:
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--shape", name, "--launches", str(args.launches),
                                  "--warmup", str(args.warmup), "--burnin", str(args.burnin)])
            if rc != 0:
                sys.exit(rc)
        return
    if not torch.cuda.is_available():
        sys.exit("sample_bench.py needs a GPU")
    one_shape(args.shape, args)


if __name__ == "__main__":
    main()
