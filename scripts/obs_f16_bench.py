#!/usr/bin/env python
"""Step and step-kernel time with the float32 and the float16 observation, same build.
Needs a GPU; not part of bench.py's metric.

    python scripts/obs_f16_bench.py [--burnin 64] [--warmup 20] [--loop 200] [--rounds 3]
                                    [--timed 100] [--out profiles/obs_f16/step_times.json]
                                    [--shapes 0,3] [--kernel auto|large|small|small2]

Per shape -- TD-def 10x10 at 65,536 / 8,192 / 4,096 boards, TD-2p 20x20 multi-action at
16,384, TD-def 30x30 at 16,384 -- one engine per format on the same seeds, each ``--burnin``
steps into a random-action rollout (the recipe of scripts/mask_bench.py) and ``--warmup``
steps warm.  Then ``--rounds`` times, alternating the formats: ``--loop`` steps between one
pair of device events (microseconds per step, launch gaps included).  Last, ``--timed``
steps with td_kernel_timing: the step kernel's own dispatch-to-end time, its median.
Reported per shape, one JSON line: both formats' step and kernel times, the kernel each
format ran, the ratio float32 / float16 of each, and beside it the bound of that ratio if
the step were nothing but its stores: (180 L^2 + 17) / (90 L^2 + 17) bytes per board
(observation + reward, done; 18,017 / 9,017 at L = 10).  ``--shapes`` picks shapes by
index, ``--kernel`` forces the step kernel of both engines (default: td_create's choice).
There is no pass mark."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))
from gym_TD.engine import TDEngine  # noqa: E402

SHAPES = [(10, 65536, "def", False), (10, 8192, "def", False), (10, 4096, "def", False),
          (20, 16384, "2p", True), (30, 16384, "def", False)]
N_BUFS = 2  # pre-drawn action batches cycled by the loop (multi-action flags are 315 MB a batch)


def make(L, B, mode, multi, dtype, args):
    seeds = np.arange(B)
    eng = TDEngine(L, B, mode, multi, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=False, obs_dtype=dtype,
                   step_kernel=args.kernel)
    eng.reset_all()
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    acts = []
    for _ in range(N_BUFS):
        d = a = None
        if mode != "atk":
            d = torch.randint(0, 3, (B, 6, L, L), generator=g, device=eng.device, dtype=torch.int64) if multi else \
                torch.randint(0, 6 * L * L + 1, (B,), generator=g, device=eng.device, dtype=torch.int64)
        if mode != "def":
            a = torch.randint(0, 5, (B, 3, 8), generator=g, device=eng.device, dtype=torch.int64)
        acts.append((d, a))
    for k in range(args.burnin + args.warmup):
        eng.step(def_act=acts[k % N_BUFS][0], atk_act=acts[k % N_BUFS][1])
    torch.cuda.synchronize()
    return eng, acts


def block(eng, acts, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(n):
        eng.step(def_act=acts[k % N_BUFS][0], atk_act=acts[k % N_BUFS][1])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def kernel_us(eng, acts, n):
    eng.kernel_timing(n)
    for k in range(n):
        eng.step(def_act=acts[k % N_BUFS][0], atk_act=acts[k % N_BUFS][1])
    torch.cuda.synchronize()
    t = eng.kernel_times()
    return float(np.median(t)), float(t.min()), int(t.size)


def shape(L, B, mode, multi, args):
    e32, a32 = make(L, B, mode, multi, torch.float32, args)
    e16, a16 = make(L, B, mode, multi, torch.float16, args)
    try:
        s32, s16 = [], []
        for _ in range(args.rounds):
            s32.append(block(e32, a32, args.loop))
            s16.append(block(e16, a16, args.loop))
        k32, k32min, n32 = kernel_us(e32, a32, args.timed)
        k16, k16min, n16 = kernel_us(e16, a16, args.timed)
        m32, m16 = float(np.median(s32)), float(np.median(s16))
        return {"L": L, "boards": B, "mode": mode, "multi_action": multi,
                "kernel_f32": e32.step_kernel_name, "kernel_f16": e16.step_kernel_name,
                "obs_MB_f32": round(e32.obs.numel() * 4 / 1e6, 1), "obs_MB_f16": round(e16.obs.numel() * 2 / 1e6, 1),
                "step_us_f32": [round(v, 2) for v in s32], "step_us_f16": [round(v, 2) for v in s16],
                "step_us_f32_median": round(m32, 2), "step_us_f16_median": round(m16, 2),
                "kernel_us_f32_median": round(k32, 2), "kernel_us_f16_median": round(k16, 2),
                "kernel_us_f32_min": round(k32min, 2), "kernel_us_f16_min": round(k16min, 2),
                "kernels_timed": [n32, n16],
                "step_ratio_f32_over_f16": round(m32 / m16, 3), "kernel_ratio_f32_over_f16": round(k32 / k16, 3),
                "store_bound_ratio": round((180.0 * L * L + 17) / (90.0 * L * L + 17), 3),
                "steps_per_block": args.loop, "burnin": args.burnin, "warmup": args.warmup}
    finally:
        e32.close()
        e16.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timed", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the records there, as a JSON list")
    ap.add_argument("--shapes", default=None, help="indices into SHAPES, comma-separated (default: all)")
    ap.add_argument("--kernel", default="auto", choices=("auto", "large", "small", "small2"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("obs_f16_bench.py needs a GPU")
    recs = []
    picked = SHAPES if args.shapes is None else [SHAPES[int(i)] for i in args.shapes.split(",")]
    for L, B, mode, multi in picked:
        recs.append(shape(L, B, mode, multi, args))
        print(json.dumps(recs[-1]), flush=True)
        if args.out:  # (after every shape: a run cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(recs, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
