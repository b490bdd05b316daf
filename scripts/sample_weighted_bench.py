#!/usr/bin/env python
"""Time of the weighted legal-action sampler (td_sample_weighted) beside the road it replaces,
the uniform sampler and a plain read of the weights.  Needs a GPU; not part of bench.py's metric.

    python scripts/sample_weighted_bench.py [--launches 50] [--warmup 10] [--burnin 64] [--shape NAME]

Per shape, in one process of its own (without --shape the script starts one child per shape,
one after the other), on boards ``--burnin`` sampled steps into a rollout, four things are timed
with a device-event pair around each of ``--launches`` calls after ``--warmup`` warm-up calls:

  a  weighted   TDEngine.sample_weighted(w) with uniform(0, 1) weights, no masses: one
                td_sample_weighted_kernel
  b  torch      the road it replaces: action_mask() + w * mask + torch.multinomial + the scatter
                into the step's formats + the gather of the chosen probability (both sides in TD-2p)
  c  uniform    TDEngine.sample_actions(): the same kernel shape without the weight read
  d  read       w.sum(1): a plain read of the weight tensor, the byte floor

The four are measured in rounds of one call each, alternating, so a drift of the machine meets
all alike.  The event pair brackets one call on an idle stream, so each figure includes the
call's own start-up, the same for all.  Shapes: 65,536 x 10x10 TD-def, 4,096 x 10x10 TD-def,
16,384 x 30x30 TD-def and 16,384 x 10x10 TD-2p.  One JSON line per shape: microseconds per call
(median, min, max, mean) of each, (a) - (c) beside (d), and whether (a)'s median lies outside
(b)'s min-max spread.  There is no pass mark."""
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
    "def10x65536": (10, 65536, "def"),
    "def10x4096": (10, 4096, "def"),
    "def30x16384": (30, 16384, "def"),
    "2p10x16384": (10, 16384, "2p"),
}


def make(L, B, mode, burnin):
    from gym_TD.engine import TDEngine
    seeds = np.arange(B)
    eng = TDEngine(L, B, mode, False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False)
    eng.reset_all()
    for k in range(burnin):
        out = eng.sample_actions(ticket=k, def_idle=0.3, atk_idle=0.3)
        eng.step(def_act=out["def"], atk_act=out["atk"])
    torch.cuda.synchronize()
    return eng


def one_shape(name, args):
    L, B, mode = SHAPES[name]
    eng = make(L, B, mode, args.burnin)
    A1 = 6 * L * L + 1
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    dw = torch.rand((B, A1), generator=g, device=eng.device, dtype=torch.float32)
    aw = torch.rand((B, 13), generator=g, device=eng.device, dtype=torch.float32) if mode != "def" else None
    four = torch.full((B, 3, 8), 4, dtype=torch.int64, device=eng.device)
    rows = torch.arange(B, device=eng.device)

    def weighted():
        eng.sample_weighted(def_w=dw, atk_w=aw)

    def road():
        m = eng.action_mask()
        p = dw * m["def"]  # (the no-op's byte is 1)
        act = torch.multinomial(p, 1)  # the step's defender format: (B,) int64
        prob = p.gather(1, act) / p.sum(1, keepdim=True)
        out = [act.reshape(B), prob]
        if aw is not None:
            legal = torch.cat([m["atk"][:, :, :4].reshape(B, 12), m["atk"][:, :1, 4]], dim=1)
            q = aw * legal
            e = torch.multinomial(q, 1).reshape(B)
            atk = four.clone()  # [3][8]: all 4 but the chosen road's first slot
            road_ = torch.clamp(e // 4, max=2)
            atk[rows, road_, 0] = torch.where(e < 12, e % 4, atk[rows, road_, 0])
            out += [atk, q.gather(1, e[:, None]) / q.sum(1, keepdim=True)]
        return out

    def uniform():
        eng.sample_actions()

    def read():
        return dw.sum(1)

    calls = {"weighted": weighted, "torch": road, "uniform": uniform, "read": read}
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
        out = {"what": "weighted sampler beside the road it replaces", "shape": name, "L": L, "boards": B, "mode": mode,
               "launches": args.launches, "kernel": eng.sample_weighted_kernel_name(), "weight_bytes": B * A1 * 4}
        for k, v in us.items():
            out[k] = {"us_median": round(float(np.median(v)), 2), "us_min": round(float(np.min(v)), 2),
                      "us_max": round(float(np.max(v)), 2), "us_mean": round(float(np.mean(v)), 2)}
        out["weighted_minus_uniform_us"] = round(out["weighted"]["us_median"] - out["uniform"]["us_median"], 2)
        out["read_us"] = out["read"]["us_median"]
        out["weighted_outside_torch_spread"] = bool(out["weighted"]["us_median"] < out["torch"]["us_min"] or
                                                    out["weighted"]["us_median"] > out["torch"]["us_max"])
        out["torch_over_weighted"] = round(out["torch"]["us_median"] / out["weighted"]["us_median"], 2)
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
        sys.exit("sample_weighted_bench.py needs a GPU")
    one_shape(args.shape, args)


if __name__ == "__main__":
    main()
