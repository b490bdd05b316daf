#!/usr/bin/env python
"""Launch and kernel time of a step at frame skip k = 1, 2, 4, 8, same build.
Needs a GPU; not part of bench.py's metric.

    python scripts/frame_skip_bench.py [--burnin 64] [--warmup 20] [--loop 200] [--rounds 3]
                                       [--timed 100] [--count 50] [--ks 1,2,4,8]
                                       [--out profiles/frame_skip/step_times.json] [--shapes 0,3]

Per shape -- TD-def 10x10 at 65,536 / 8,192 / 4,096 boards and TD-def 30x30 at 16,384 in
float32, and 10x10 at 65,536 in float16 -- one engine per k on the same seeds, each
``--burnin`` launches into a random-action rollout and ``--warmup`` launches warm.  Then
``--rounds`` times, alternating the engines: ``--loop`` launches between one pair of device
events (microseconds per launch, launch gaps included).  Then ``--timed`` launches with
td_kernel_timing: the kernel's own dispatch-to-end time, its median.  Last, ``--count``
launches that add up what the boards' step counters advanced by (ep_len against the count
before the launch): a board that finishes its episode at sub-step j runs j + 1 of its k
sub-steps, so the board steps per launch are fewer than B k -- the rate reported counts
the sub-steps actually executed.  One JSON line per shape: per k the kernel, microseconds
per launch (every block and the median), the kernel's median, executed sub-steps per
launch, board steps per second, and its ratio to k = 1 beside the bound k.  There is no
pass mark."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "gym-td_amd"))
from gym_TD.engine import TDEngine  # noqa: E402

SHAPES = [(10, 65536, torch.float32), (10, 8192, torch.float32), (10, 4096, torch.float32),
          (30, 16384, torch.float32), (10, 65536, torch.float16)]
N_BUFS = 2  # pre-drawn action batches cycled by the loop


def make(L, B, dtype, k, args):
    seeds = np.arange(B)
    eng = TDEngine(L, B, "def", False, 1, np_seeds=seeds, py_seeds=seeds, autoreset=True, info=True, obs_dtype=dtype,
                   frame_skip=k)
    eng.reset_all()
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    acts = [torch.randint(0, 6 * L * L + 1, (B,), generator=g, device=eng.device, dtype=torch.int64)
            for _ in range(N_BUFS)]
    for i in range(args.burnin + args.warmup):
        eng.step(def_act=acts[i % N_BUFS])
    torch.cuda.synchronize()
    return eng, acts


def block(eng, acts, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        eng.step(def_act=acts[i % N_BUFS])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def kernel_us(eng, acts, n):
    eng.kernel_timing(n)
    for i in range(n):
        eng.step(def_act=acts[i % N_BUFS])
    torch.cuda.synchronize()
    t = eng.kernel_times()
    return float(np.median(t)), float(t.min()), int(t.size)


def executed(eng, acts, n):
    """Board steps per launch over n launches, from the boards' step counters."""
    torch.cuda.synchronize()
    before = torch.from_numpy(eng.export_state()["hdr"]["steps"].astype(np.int64)).to(eng.device)
    total = torch.zeros((), dtype=torch.int64, device=eng.device)
    for i in range(n):
        eng.step(def_act=acts[i % N_BUFS])
        ran = eng.ep_len.to(torch.int64) - before  # ep_len: the counter after the last executed sub-step
        total += ran.sum()
        before = torch.where(eng.done != 0, torch.zeros_like(before), eng.ep_len.to(torch.int64))
    return float(total.item()) / n


def shape(L, B, dtype, args):
    ks = [int(k) for k in args.ks.split(",")]
    engs = [make(L, B, dtype, k, args) for k in ks]
    try:
        times = [[] for _ in ks]
        for _ in range(args.rounds):
            for i, (e, a) in enumerate(engs):
                times[i].append(block(e, a, args.loop))
        rec = {"L": L, "boards": B, "mode": "def", "obs": "float16" if dtype == torch.float16 else "float32",
               "launches_per_block": args.loop, "burnin": args.burnin, "warmup": args.warmup, "k": {}}
        base = None
        for k, (e, a), t in zip(ks, engs, times):
            kus, kmin, n = kernel_us(e, a, args.timed)
            ran = executed(e, a, args.count)
            med = float(np.median(t))
            rate = ran / (med * 1e-6)
            base = rate if k == 1 else base
            rec["k"][str(k)] = {"kernel": e.step_kernel_name, "launch_us": [round(v, 2) for v in t],
                                "launch_us_median": round(med, 2), "kernel_us_median": round(kus, 2),
                                "kernel_us_min": round(kmin, 2), "kernels_timed": n,
                                "board_steps_per_launch": round(ran, 1), "executed_fraction": round(ran / (B * k), 4),
                                "board_steps_per_s": round(rate, 1), "us_per_board_step_x_B": round(med * B / ran, 2),
                                "ratio_to_k1": None if base is None else round(rate / base, 3), "bound": k}
        return rec
    finally:
        for e, _ in engs:
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--burnin", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timed", type=int, default=100)
    ap.add_argument("--count", type=int, default=50)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--out", default=None, help="also write the records there, as a JSON list")
    ap.add_argument("--shapes", default=None, help="indices into SHAPES, comma-separated (default: all)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_skip_bench.py needs a GPU")
    recs = []
    picked = SHAPES if args.shapes is None else [SHAPES[int(i)] for i in args.shapes.split(",")]
    for L, B, dtype in picked:
        recs.append(shape(L, B, dtype, args))
        print(json.dumps(recs[-1]), flush=True)
        if args.out:  # (after every shape: a run cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(recs, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
